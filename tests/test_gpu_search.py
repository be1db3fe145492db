"""The column search on the device: ``atx_search_columns`` equals the numpy loop of include/atx_search.h (tests/search_statement.py) bit for
bit — NaN where the loop has NaN — lies within the header's bound of the exact statement, gives the loop's ``count``, the same bytes in
every storage shape and writes nothing beyond a point's rows; then the refusal at 257 levels, ``vertical.search_columns`` where the
variables overflow a workgroup's LDS, and the two filters end to end."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import search_statement as ss
from anemoi_transform_amd import native_search
from anemoi_transform_amd.fields import fieldlist_from_dicts
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.grids import lookup
from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack
from anemoi_transform_amd.vertical import search_columns
from hybrid_column_common import CANARY, WIDTHS, allocate, assert_same_bits

pytestmark = pytest.mark.gpu

STORAGE = ("columns", "columns-pitch+1", "fields-pitch+3")  # the 16-byte routes where the shape allows, the scalar routes, the field-major kernel


def run_kernel(dev, T, shape, storage: str, direction: str, mode: str):
    """The kernel on the shared case in one storage shape: ``(y [n_pts, n_out, n_tgt], count [n_pts, n_tgt])`` after asserting that
    everything of the output's allocation but a point's rows (a row's ``n_pts`` points), and of the count's but its bytes, is untouched."""
    s, x, targets, level_values = ss.case(np.dtype(T).name, shape)
    n_pts, n_var, n_lev = x.shape
    n_tgt = 1 if mode in ss.EXTREMA else len(targets)
    n_out = n_var + (level_values is not None)
    columns = storage.startswith("columns")
    rows = dict(src=n_var * n_lev, search=n_lev, out=n_out * n_tgt)
    values = dict(src=x.reshape(n_pts, -1), search=s)
    stacks = {}
    for name, n in rows.items():
        stacks[name] = allocate(*((n_pts, n) if columns else (n, n_pts)), storage, T, dev, CANARY if name == "out" else float("nan"))
        if name != "out" and n:
            stacks[name][:, : n if columns else n_pts] = torch.from_numpy(np.ascontiguousarray(values[name] if columns else values[name].T)).to(dev)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    count = torch.full((n_pts * n_tgt + 16,), 7, dtype=torch.uint8, device=dev)
    native_search.columns(stacks["src"] if n_var else None, stacks["search"], stacks["out"], None if mode in ss.EXTREMA else up(targets), n_pts=n_pts,
                          n_var=n_var, n_lev=n_lev, n_tgt=n_tgt, src_pitch=stacks["src"].shape[1], search_pitch=stacks["search"].shape[1],
                          out_pitch=stacks["out"].shape[1], layout=COLUMNS if columns else FIELDS, direction=direction, mode=mode,
                          level_values=up(level_values), count=count[: n_pts * n_tgt])
    torch.cuda.synchronize()
    width = rows["out"] if columns else n_pts
    host = stacks["out"]._base.cpu().numpy().copy()
    view = host[: stacks["out"].numel()].reshape(stacks["out"].shape)
    got = view[:, :width].copy()
    view[:, :width] = CANARY
    assert (host == CANARY).all() and (count[n_pts * n_tgt:] == 7).all(), f"{shape} {storage}: written beyond a row"
    counted = count[: n_pts * n_tgt].cpu().numpy()
    return ((got if columns else np.ascontiguousarray(got.T)).reshape(n_pts, n_out, n_tgt),
            counted.reshape(n_pts, n_tgt) if columns else np.ascontiguousarray(counted.reshape(n_tgt, n_pts).T))


@pytest.mark.parametrize("shape", ss.SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("T", WIDTHS)
def test_the_kernel_is_the_statement_bit_for_bit_in_every_storage(dev, T, shape):
    s, x, _, level_values = ss.case(np.dtype(T).name, shape)
    for direction in (ss.FORWARD, ss.BACKWARD):
        for mode in ss.CROSSINGS + ss.EXTREMA:
            want, want_count, crossing = ss.reference(np.dtype(T).name, shape, direction, mode)
            first = None
            for storage in STORAGE:
                got, count = run_kernel(dev, T, shape, storage, direction, mode)
                assert_same_bits(got, want, f"{shape} {storage} {direction} {mode}", "(point, variable, target)")
                assert np.array_equal(count, want_count), f"{shape} {storage} {direction} {mode}: count differs at {np.argwhere(count != want_count)[:5].tolist()}"
                first = got if first is None else first
                assert got.tobytes() == first.tobytes(), f"{shape} {direction} {mode}: {storage} differs from {STORAGE[0]}"
            worst = ss.worst_ulps(first, s, x, crossing, level_values)
            print(f"search kernel {np.dtype(T).name} {shape} {direction} {mode}: {worst:.4f} ulps from exact, bound {ss.bound(T):.9g}")
            assert worst <= ss.bound(T)


def test_257_levels_are_refused(dev):
    s = Stack.from_fields(list(np.zeros((257, 8))), dev=dev)
    with pytest.raises(NotImplementedError, match="n_lev=257 exceeds the 256 levels of one call"):
        search_columns(s, s, [0.5], n_var=1)


def test_variables_beyond_a_workgroups_lds_are_halved_with_the_same_bits(dev, monkeypatch):
    """80 float64 variables of 128 levels are 80 KiB a point: the column kernel refuses them, ``search_columns`` launches two halves into
    the one result — level_values with the second, the count with the first — and every variable has the bits of its own launch."""
    n_pts, n_lev, n_var = 40, 128, 80
    rng = np.random.default_rng(5)
    s = rng.integers(0, 8, (n_pts, n_lev)).astype(np.float64)
    x = rng.standard_normal((n_pts, n_var, n_lev))
    targets, levels = [3.5, 0.25, 7.0], np.arange(1.0, n_lev + 1)
    stack, search = Stack.from_fields(list(x.reshape(n_pts, -1).T), dev=dev), Stack.from_fields(list(s.T), dev=dev)
    launches, real = [], native_search.columns
    monkeypatch.setattr(native_search, "columns", lambda *a, **k: (launches.append((k["n_var"], k["level_values"] is not None, k["count"] is not None)),
                                                                   real(*a, **k))[1])
    out, count = search_columns(stack, search, targets, n_var=n_var, direction="backward", mode="down", level_values=levels, count=True)
    assert launches == [(80, True, True), (40, False, True), (40, True, False)]
    got = out.numpy().reshape(n_var + 1, len(targets), n_pts)
    for v in range(n_var):
        single, _ = search_columns(Stack(stack.data[:, v * n_lev:(v + 1) * n_lev], n_pts, n_lev, COLUMNS), search, targets, direction="backward", mode="down")
        assert single.numpy().tobytes() == got[v].tobytes(), v
    want, want_count, _ = ss.statement(s, x, np.array(targets), ss.BACKWARD, ss.DOWN, levels)
    assert_same_bits(np.ascontiguousarray(got.transpose(2, 0, 1)), want, "halved launches", "(point, variable, target)")
    assert np.array_equal(count.cpu().numpy(), want_count)


# ---- the filters, end to end -------------------------------------------------------------------------------------------------------------
LEVELS_HPA = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
DATES = (20260101, 20260102)


def small_world(dtype):
    """684 points (more than one workgroup in either layout), two dates, 13 pressure levels in no order: ``t`` with inversions and NaN
    under the ground, a wind speed ``ws``, and ``z`` / ``u``.  ``truth[date]``: ``{param: [n_pts, 13]}`` in the order of LEVELS_HPA."""
    grid = lookup([10.0, 10.0])
    lat, lon = np.asarray(grid["latitudes"], dtype=np.float64), np.asarray(grid["longitudes"], dtype=np.float64)
    n, rng, specs, truth = len(lat), np.random.default_rng(31), [], {}
    for date in DATES:
        common = dict(latitudes=lat, longitudes=lon, date=date, time=0, step=0)
        columns = dict(t=(215.0 + 6.0 * np.arange(13) + 9.0 * rng.standard_normal((n, 13))).astype(dtype), ws=rng.integers(0, 40, (n, 13)).astype(dtype),
                       z=np.cumsum(rng.uniform(800.0, 30000.0, (n, 13)), axis=1)[:, ::-1].astype(dtype), u=(20.0 * rng.standard_normal((n, 13))).astype(dtype))
        columns["t"][::9, 11:] = np.nan  # under the ground
        for k in rng.permutation(13):
            for param in ("u", "t", "z", "ws"):
                specs.append(dict(values=columns[param][:, k].copy(), param=param, levtype="pl", levelist=LEVELS_HPA[k], **common))
        truth[date] = columns
    return fieldlist_from_dicts(specs, mars=True), truth


def run_filter(f, data, monkeypatch):
    launches, real = [], native_search.columns
    monkeypatch.setattr(native_search, "columns", lambda *a, **k: (launches.append((k["n_var"], k["n_lev"], k["n_tgt"])), real(*a, **k))[1])
    result, kept = list(f.forward(data)), list(data)
    assert all(a is b for a, b in zip(result, kept))  # every input passes through
    new = result[len(kept):]
    assert all(g.metadata("levtype") == "sfc" and g.stack_ref()[0].data.is_cuda for g in new) and len({id(g.stack_ref()[0]) for g in new}) == len(DATES)
    return launches, new


@pytest.mark.parametrize("T", WIDTHS)
def test_crossing_level_end_to_end(dev, monkeypatch, T):
    data, truth = small_world(T)
    f = create_filter_by_name("crossing_level", search="t", values=[273.15, 253.15], start="ground", sense="any",
                              outputs={"deg": "z", "pdeg": "levelist"}, count="ndeg")
    launches, new = run_filter(f, data, monkeypatch)
    assert launches == [(1, 13, 2)] * len(DATES)  # ONE launch per group
    names = ["deg_273.15", "deg_253.15", "pdeg_273.15", "pdeg_253.15", "ndeg_273.15", "ndeg_253.15"]
    assert [(g.metadata("date"), g.metadata("param")) for g in new] == [(date, name) for date in DATES for name in names]
    for i, date in enumerate(DATES):
        c = truth[date]
        got = np.stack([g.to_numpy(flatten=True) for g in new[i * 6:(i + 1) * 6]], axis=1).reshape(-1, 3, 2)
        want, count, _ = ss.statement(c["t"], c["z"][:, None, :], np.array([273.15, 253.15]), ss.BACKWARD, ss.ANY, np.array(LEVELS_HPA, dtype=np.float64))
        assert got.dtype == T and (count > 1).any() and (count == 0).any()
        assert_same_bits(got[:, :2], want, f"crossing_level {date}", "(point, variable, target)")
        assert np.array_equal(got[:, 2], count.astype(T))


@pytest.mark.parametrize("T", WIDTHS)
def test_extremum_level_end_to_end(dev, monkeypatch, T):
    data, truth = small_world(T)
    f = create_filter_by_name("extremum_level", search="ws", kind="maximum", start="top", outputs={"zjet": "z", "ujet": "u", "wsjet": "ws"})
    launches, new = run_filter(f, data, monkeypatch)
    assert launches == [(3, 13, 1)] * len(DATES)
    assert [(g.metadata("date"), g.metadata("param")) for g in new] == [(date, name) for date in DATES for name in ("zjet", "ujet", "wsjet")]
    for i, date in enumerate(DATES):
        c = truth[date]
        got = np.stack([g.to_numpy(flatten=True) for g in new[i * 3:(i + 1) * 3]], axis=1).reshape(-1, 3, 1)
        want, count, _ = ss.statement(c["ws"], np.stack([c["z"], c["u"], c["ws"]], axis=1), None, ss.FORWARD, ss.MAX)
        assert got.dtype == T and (count > 1).any()
        assert_same_bits(got, want, f"extremum_level {date}", "(point, variable, target)")
