"""``atx_search_columns`` without a GPU: the numpy loop of include/atx_search.h (tests/search_statement.py) against the same statement in
exact arithmetic, within the header's bound, on columns whose answers are read off by eye, and the shares of its random cases; then the C
ABI's argument validation through ctypes and what the two filters refuse, name and map."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import search_statement as ss
from anemoi_transform_amd import native, native_search
from anemoi_transform_amd.filters import create_filter_by_name
from hybrid_column_common import WIDTHS, fields

nan, inf = np.nan, np.inf


@pytest.mark.parametrize("shape", ss.SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("T", WIDTHS)
def test_the_loop_is_within_the_headers_bound_and_its_cases_have_every_kind(T, shape):
    name = np.dtype(T).name
    s, x, targets, level_values = ss.case(name, shape)
    for direction in (ss.FORWARD, ss.BACKWARD):
        for mode in ss.CROSSINGS:
            y, count, crossing = ss.reference(name, shape, direction, mode)
            worst = ss.worst_ulps(y, s, x, crossing, level_values)
            print(f"search {name} {shape} {direction} {mode}: numpy {worst:.4f} ulps from exact over {len(crossing)} crossings, bound {ss.bound(T):.9g}")
            assert worst <= ss.bound(T) and native_search.ULPS_F64 == ss.ULPS_F64
        # the random remainder (not the points by hand, not the NaN target) under "any": with, without and with several crossings
        count = ss.reference(name, shape, direction, ss.ANY)[1][ss.PLANTED if len(s) > 16 else 0:][:, ~np.isnan(targets)]
        if shape[1] >= 3 and count.size >= 30:
            assert (count > 0).mean() >= 0.5 and (count == 0).mean() >= 0.1 and (count > 1).mean() >= 0.1, (direction, (count > 0).mean(), (count > 1).mean())
    if len(s) > 16 and shape[1] >= 6:  # the points by hand say what their docstring says, read forward
        count = ss.reference(name, shape, ss.FORWARD, ss.ANY)[1][:, 0]
        assert count[:8].tolist() == [0, 1, 1, 1, 1, 0, 1, 3] and count[10] == 0
        y = ss.reference(name, shape, ss.FORWARD, ss.UP)[0]
        assert np.isnan(y[0, :, 0]).all() and np.isnan(y[10]).all() and not np.isnan(y[5, :, 0]).any()  # 5: the last level alone equals T
        assert [ss.reference(name, shape, d, ss.ANY)[1][p, 0] > 0 for d, p in ((ss.FORWARD, 8), (ss.BACKWARD, 9))] == [True, True]
        for mode in ss.EXTREMA:
            assert ss.reference(name, shape, ss.FORWARD, mode)[1][12, 0] == 2 and ss.reference(name, shape, ss.FORWARD, mode)[1][10, 0] == 0


def test_the_loop_gives_answers_read_off_by_eye():
    s = np.array([[1.0, 3.0, 2.0, 0.0, 4.0]])  # rises, falls twice, rises
    x = np.array([[[10.0, 30.0, 20.0, 0.0, 40.0]]])
    levels = np.array([100.0, 200.0, 300.0, 400.0, 500.0])
    run = lambda targets, d, m, col=s: ss.statement(col, x, np.array(targets), d, m, levels)  # noqa: E731
    y, count, _ = run([2.5, 3.0, 5.0, 4.0, nan], ss.FORWARD, ss.ANY)
    # 2.5: step 0 -> 1, three quarters of the way;  3.0 ON level 1 is where the DOWN step 1 -> 2 starts (w == 0), step 0 -> 1 does not reach it;
    # 5.0: nothing;  4.0: no step (the compare with the far end is strict) but the last level equals it;  NaN: nothing
    assert np.array_equal(y[0, 0], [25.0, 30.0, nan, 40.0, nan], equal_nan=True) and np.array_equal(y[0, 1], [175.0, 200.0, nan, 500.0, nan], equal_nan=True)
    assert count[0].tolist() == [3, 2, 0, 0, 0]
    assert run([2.5], ss.FORWARD, ss.DOWN)[0][0, :, 0].tolist() == [25.0, 250.0] and run([2.5], ss.FORWARD, ss.DOWN)[1][0, 0] == 1
    # from the far end "rising" is read along the scan: 4 -> 0 falls through 2.5 first, 0 -> 2 is the first to rise
    assert run([2.5], ss.BACKWARD, ss.ANY)[0][0, 0, 0] == 40.0 + (2.5 - 4.0) / (0.0 - 4.0) * (0.0 - 40.0)
    assert run([1.0], ss.BACKWARD, ss.UP)[0][0, :, 0].tolist() == [10.0, 350.0] and run([1.0], ss.BACKWARD, ss.UP)[1][0, 0] == 1
    assert run([1.0], ss.BACKWARD, ss.ANY)[1][0, 0] == 2  # (4 -> 0 and 0 -> 2;  3 -> 1 only REACHES 1.0: the compare with the far end is strict)
    # the extremum: the first among equals in scan order, NaN apart; all NaN is NaN
    two = np.array([[nan, 4.0, 1.0, 4.0, nan]])
    assert run(None, ss.FORWARD, ss.MAX, two)[0][0, :, 0].tolist() == [30.0, 200.0] and run(None, ss.BACKWARD, ss.MAX, two)[0][0, :, 0].tolist() == [0.0, 400.0]
    assert run(None, ss.FORWARD, ss.MAX, two)[1][0, 0] == 2 and run(None, ss.FORWARD, ss.MIN, two)[0][0, :, 0].tolist() == [20.0, 300.0]
    y, count, _ = run(None, ss.FORWARD, ss.MIN, np.full((1, 5), nan))
    assert np.isnan(y).all() and count[0, 0] == 0
    # NaN levels are skipped, not fatal; an infinity is the plain result of the formula
    holed = np.array([[nan, nan, 2.0, 0.0, 4.0]])
    assert run([1.0], ss.FORWARD, ss.ANY, holed)[0][0, 0, 0] == 10.0 and np.isnan(run([3.0], ss.BACKWARD, ss.DOWN, np.array([[nan, 3.5, nan, 2.0, nan]]))[0]).all()
    assert run([1.0], ss.FORWARD, ss.UP, np.array([[0.0, inf, 0.0, 0.0, 0.0]]))[0][0, 0, 0] == 10.0  # w = 1 / inf = 0
    assert np.isnan(run([1.0], ss.FORWARD, ss.UP, np.array([[-inf, 2.0, 0.0, 0.0, 0.0]]))[0][0, 0, 0])  # w = inf / inf
    one = ss.statement(np.array([[7.0]]), np.array([[[3.0]]]), np.array([7.0, 8.0]), ss.FORWARD, ss.ANY)[0]
    assert np.array_equal(one[0, 0], [3.0, nan], equal_nan=True)


def test_abi_argument_validation_without_a_gpu():
    """Every refusal of include/atx_search.h comes before anything touches HIP: the device pointers are never dereferenced."""
    lib = native_search.load()
    assert lib.atx_search_version() == 420 and native_search.MAX_LEVELS == 256
    assert native_search.MODES == dict(up=0, down=1, any=2, max=3, min=4) and native_search.DIRECTIONS == dict(forward=0, backward=1)
    at = lambda address: ctypes.c_void_p(address)  # noqa: E731

    def call(src=at(1 << 20), search=at(2 << 20), out=at(3 << 20), count=None, targets=at(80), level_values=None, n_pts=0, n_var=2, n_lev=4, n_tgt=3,
             src_pitch=8, search_pitch=4, out_pitch=6, dtype=0, layout=0, direction=0, mode=2):
        return lib.atx_search_columns(src, search, out, count, targets, level_values, n_pts, n_var, n_lev, n_tgt, src_pitch, search_pitch, out_pitch, dtype,
                                      layout, direction, mode, None)

    said = lambda: lib.atx_search_last_error().decode()  # noqa: E731
    name = "atx_search_columns"
    assert call() == native.OK and call(src=None, search=None, out=None) == native.OK and call(n_pts=8, n_tgt=0, targets=None, out=None) == native.OK
    assert call(dtype=7) == native.EINVAL and said() == f"{name}: bad dtype 7"
    assert call(layout=5) == native.EINVAL and said() == f"{name}: bad layout 5"
    assert call(direction=2) == native.EINVAL and said() == f"{name}: unknown direction 2"
    assert call(mode=5) == native.EINVAL and said() == f"{name}: unknown mode 5"
    for wrong in (dict(n_pts=-1), dict(n_var=-1), dict(n_lev=0), dict(n_tgt=-1)):
        assert call(**wrong) == native.EINVAL and "bad sizes" in said()
    assert call(mode=3) == native.EINVAL and "an extremum has one result" in said() and call(mode=4, n_tgt=1, targets=None) == native.OK
    assert call(n_var=0, src=None, src_pitch=0) == native.EINVAL and "nothing would be written" in said()
    assert call(n_var=0, src=None, src_pitch=0, count=at(1 << 30)) == native.OK and call(n_var=0, src=None, src_pitch=0, out_pitch=3, level_values=at(1 << 30)) == native.OK
    assert call(targets=None) == native.EINVAL and said() == f"{name}: null targets"
    for arg, least in (("src_pitch", 8), ("search_pitch", 4), ("out_pitch", 6)):
        assert call(**{arg: least - 1}) == native.ESHAPE and "column pitch" in said() and "< rows (8, 4, 6)" in said()
    assert call(level_values=at(1 << 30), out_pitch=8) == native.ESHAPE and "< rows (8, 4, 9)" in said()
    assert call(layout=1, n_pts=0, search_pitch=-1) == native.ESHAPE and "field pitch" in said()
    assert call(n_lev=257, src_pitch=514, search_pitch=257) == native.ENOTIMPL and "exceeds the 256 levels of one call" in said()
    assert call(n_tgt=32768, out_pitch=1 << 20) == native.ENOTIMPL and "exceed the indexing" in said()
    assert call(n_pts=2**31) == native.ENOTIMPL
    # with points: null pointers and overlap are refused, and one point beyond the LDS of a workgroup, all before the launch
    for arg in ("src", "search"):
        assert call(n_pts=8, **{arg: None}) == native.EINVAL and said() == f"{name}: null src / search pointer"
    assert call(n_pts=8, out=None) == native.EINVAL and said() == f"{name}: null out pointer"
    assert call(n_pts=8, out=at((1 << 20) + 100)) == native.EINVAL and said() == f"{name}: out overlaps src"
    assert call(n_pts=8, out=at((2 << 20) - 100)) == native.EINVAL and said() == f"{name}: out overlaps search"
    assert call(n_pts=8, out=at(90)) == native.EINVAL and said() == f"{name}: out overlaps targets"
    assert call(n_pts=8, level_values=at(1 << 30), out_pitch=9, count=at((1 << 30) + 31)) == native.EINVAL and said() == f"{name}: count overlaps level_values"
    assert call(n_pts=8, count=at((3 << 20) + 8)) == native.EINVAL and said() == f"{name}: count overlaps out"
    assert call(n_pts=8, n_var=1, src_pitch=4, n_tgt=20000, out_pitch=20000, out=at(1 << 40)) == native.ENOTIMPL and "bytes of LDS" in said()


def test_the_filters_check_their_configuration_and_name_their_outputs():
    f = create_filter_by_name("crossing_level", search="t", values=[273.15, 263], outputs={"deg": "z", "pdeg": "levelist", "udeg": "u"}, count="n")
    assert (f.values, f.mode, f.direction, f.variables, f.with_levelist) == ([273.15, 263], "any", "backward", ["z", "u"], True)
    assert f.output_names() == ["deg_273.15", "deg_263", "pdeg_273.15", "pdeg_263", "udeg_273.15", "udeg_263", "n_273.15", "n_263"]
    assert create_filter_by_name("crossing_level", outputs={"deg0l": "z"}, count="n").output_names() == ["deg0l", "n"]
    g = create_filter_by_name("extremum_level", search="ws", kind="minimum", start="top", outputs={"zjet": "z"})
    assert (g.mode, g.direction, g.values, g.output_names()) == ("min", "forward", [], ["zjet"])
    # the ground is the largest levelist on pl and ml, the smallest on hl; rising and falling are read along the scan
    for levtype, start, direction in (("pl", "ground", "backward"), ("pl", "top", "forward"), ("ml", "ground", "backward"), ("ml", "top", "forward"),
                                      ("hl", "ground", "forward"), ("hl", "top", "backward")):
        assert create_filter_by_name("crossing_level", outputs={"a": "z"}, levtype=levtype, start=start).direction == direction
    assert [create_filter_by_name("crossing_level", outputs={"a": "z"}, sense=s).mode for s in ("any", "rising", "falling")] == ["any", "up", "down"]
    for name, wrong, message in (("crossing_level", dict(outputs={"a": "z"}, start="sky"), "start must be one of 'ground', 'top'"),
                                 ("crossing_level", dict(outputs={"a": "z"}, sense="sideways"), "sense must be one of 'any', 'rising', 'falling'"),
                                 ("crossing_level", dict(outputs={"a": "z"}, values=["cold"]), "values must be numbers"),
                                 ("crossing_level", dict(outputs={"a": "z"}, values=[]), "non-empty list"),
                                 ("crossing_level", dict(outputs={"a": "z"}, values=[1, 1.0]), "duplicate values"),
                                 ("crossing_level", dict(outputs={"a": "z"}, levtype="sfc"), "levtype must be one of"),
                                 ("crossing_level", dict(), "nothing would be written"), ("crossing_level", dict(outputs={"a": "z"}, count="a"), "also one of the outputs"),
                                 ("extremum_level", dict(outputs={"a": "z"}, kind="median"), "kind must be one of 'maximum', 'minimum'"),
                                 ("extremum_level", dict(outputs={"a": "z"}, values=[1.0]), "an extremum takes no values"),
                                 ("extremum_level", dict(outputs=["z"]), "outputs must be a dict")):
        with pytest.raises(ValueError, match=f"{name}: .*{message}"):
            create_filter_by_name(name, **wrong)
    assert (f | g).filters == [f, g]  # a | b builds a pipeline


T3, Z3 = [("t", "pl", k) for k in (500, 850, 1000)], [("z", "pl", k) for k in (500, 850, 1000)]


def test_grouping_errors_come_before_any_launch():
    """Host fields, no GPU here: each of these raises from the bookkeeping, before a stack is built or a kernel launched."""
    f = create_filter_by_name("crossing_level", search="t", outputs={"deg0l": "z", "p0": "levelist"})
    for specs, message in (((*Z3,), "no fields of the search param 't' on levtype 'pl'"), ((*T3,), "no fields of the output param 'z' on levtype 'pl'"),
                           ((*T3, *Z3[1:]), r"mixed level sets for t and z: \[500, 850, 1000\] and \[850, 1000\]"),
                           ((*T3, T3[1], *Z3), "Duplicate component t .* level 850")):
        with pytest.raises(ValueError, match=message):
            f.forward(fields(*specs))
    data = list(fields(T3[2], Z3[0], T3[0], Z3[2], Z3[1], T3[1], ("t", "ml", 3), ("2t", "sfc", None)))  # t on ml and 2t are not this filter's
    passed, (group,) = f._plan(data)
    assert all(a is b for a, b in zip(passed, data)) and len(passed) == len(data) and group["levels"] == [500, 850, 1000]
    assert [x.metadata("levelist") for x in group["by_param"]["t"]] == [500, 850, 1000] == [x.metadata("levelist") for x in group["by_param"]["z"]]
    assert f._plan(list(fields(("2t", "sfc", None))))[1] == []
