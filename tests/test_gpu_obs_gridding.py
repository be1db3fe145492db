"""Observation gridding on the device: ``atx_obs_best_per_cell`` + ``atx_obs_fill_stack`` (csrc/atx_obs.hip) against the numpy
restatement (tests/obs_gridding_restatement.py), and ``irregular_to_grid`` / ``assign_to_grid`` through the plugin API on the golden
cases (tests/golden/irregular_to_grid.json).  Equality everywhere: a winner is chosen and its values are copied."""

from __future__ import annotations

import datetime
import zlib

import numpy as np
import pytest
import torch

from anemoi_transform_amd import native, obs
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.filters.tabular import IrregularToGrid
from anemoi_transform_amd.grids import lookup
from anemoi_transform_amd.stack import COLUMNS, FIELDS

import obs_gridding_restatement as R

pytestmark = pytest.mark.gpu

GOLDEN = R.load_golden()
MINUTE = 60 * 10**9
H = 60 * MINUTE
BASE = int(np.datetime64("2024-03-01T00:00", "ns").astype(np.int64))
I64 = np.iinfo(np.int64)


def random_table(rng, n, n_cells, n_cols, n_time, spacing_min=360, specials=True):
    """Dates on a one-minute lattice (ties are common), NaT rows, all-NaN and partly-NaN rows, cells outside the grid."""
    date = BASE + rng.integers(0, (n_time + 1) * spacing_min, n) * MINUTE
    cell = rng.integers(0, max(n_cells, 1), n).astype(np.int64)
    values = rng.integers(0, 1000, (n_cols, n)).astype(np.float64) + 0.25
    values[rng.random((n_cols, n)) < 0.25] = np.nan
    if specials and n >= 40:
        date[rng.integers(0, n, 5)] = I64.min
        values[:, rng.integers(0, n, n // 10)] = np.nan
        cell[rng.integers(0, n, 8)] = [-1, n_cells, I64.min, I64.max, n_cells + 1, -2, 2**31, 2**32 + 1]
        crowd = rng.integers(0, n, n // 3)  # a few crowded cells: equal scores within a cell
        cell[crowd] = rng.integers(0, min(3, n_cells), len(crowd))
    targets = BASE + np.arange(1, n_time + 1, dtype=np.int64) * spacing_min * MINUTE
    return date, cell, values, targets


def device_run(date, cell, values, targets, n_cells, window, freq_ns, weight, layout):
    stack, winner = obs.grid_observations(date, cell, values, targets, n_cells=n_cells, window=obs.Window(*window), freq=freq_ns,
                                          weight=weight, layout=layout, return_winner=True)
    torch.cuda.synchronize()
    return stack, winner


def check(date, cell, values, targets, n_cells, window, freq_ns, weight, layout):
    want, want_winner = R.grid_observations(date, cell, values, targets, n_cells, window, freq_ns, weight)
    stack, winner = device_run(date, cell, values, targets, n_cells, window, freq_ns, weight, layout)
    np.testing.assert_array_equal(winner.cpu().numpy(), want_winner)
    assert stack.n_lev == len(targets) * len(values) and stack.n_pts == n_cells and stack.dtype == torch.float64
    np.testing.assert_array_equal(stack.numpy(), want)
    return want_winner


@pytest.mark.parametrize("layout", [COLUMNS, FIELDS], ids=["columns", "fields"])
@pytest.mark.parametrize("n_time, n_cols", [(1, 1), (4, 3), (33, 8), (4, 8), (33, 1), (1, 3)])
def test_kernels_equal_the_restatement(dev, layout, n_time, n_cols):
    rng = np.random.default_rng(zlib.crc32(f"{layout}-{n_time}-{n_cols}".encode()))
    n_cells = int(rng.choice([61, 257, 1001]))  # not multiples of the vector width
    n = 20000
    date, cell, values, targets = random_table(rng, n, n_cells, n_cols, n_time)
    closed = [(False, True), (True, True), (False, False), (True, False)][(n_time + n_cols) % 4]
    weight = [0.0, 0.3, 1.0][(n_time * 3 + n_cols) % 3]
    winner = check(date, cell, values, targets, n_cells, (-9 * H, 3 * H, *closed), 6 * H, weight, layout)
    assert (winner >= 0).mean() > 0.3


@pytest.mark.parametrize("closed_before", [False, True])
@pytest.mark.parametrize("closed_after", [False, True])
@pytest.mark.parametrize("weight", [0.0, 0.3, 1.0])
def test_window_ends_and_weights(dev, closed_before, closed_after, weight):
    rng = np.random.default_rng(7 + 2 * closed_before + closed_after)
    # dates on the targets' own lattice: many rows sit exactly on a window end
    n, n_cells, n_time = 6000, 97, 4
    date, cell, values, targets = random_table(rng, n, n_cells, 3, n_time)
    on_end = rng.integers(0, n, n // 2)
    date[on_end] = BASE + rng.integers(0, n_time + 2, len(on_end)) * 180 * MINUTE
    for layout in (COLUMNS, FIELDS):
        check(date, cell, values, targets, n_cells, (-6 * H, 3 * H, closed_before, closed_after), 6 * H, weight, layout)


@pytest.mark.parametrize("layout", [COLUMNS, FIELDS], ids=["columns", "fields"])
def test_empty_table_gives_an_all_nan_stack(dev, layout):
    targets = BASE + np.arange(1, 4, dtype=np.int64) * 6 * H
    empty = np.zeros(0, dtype=np.int64)
    stack, winner = device_run(empty, empty, np.zeros((2, 0)), targets, 11, (-6 * H, 0, False, True), 6 * H, 0.3, layout)
    assert (winner.cpu().numpy() == -1).all() and winner.shape == (3, 11)
    got = stack.numpy()
    assert got.shape == (6, 11) and np.isnan(got).all()
    # and no targets at all: a stack of no levels
    stack, winner = device_run(empty, empty, np.zeros((2, 0)), empty, 11, (-6 * H, 0, False, True), 6 * H, 0.0, layout)
    assert stack.n_lev == 0 and winner.numel() == 0


def test_rows_that_never_take_part(dev):
    """NaT rows, all-NaN rows and cells at -1, n_cells, INT64_MIN, INT64_MAX are skipped, not dereferenced: alone in a table they
    leave every cell empty; next to good rows they change nothing."""
    n_cells, target = 5, np.array([BASE + 6 * H])
    date = np.full(8, BASE + 5 * H)
    cell = np.array([-1, n_cells, I64.min, I64.max, 2, 3, 0, 1], dtype=np.int64)
    values = np.arange(16, dtype=np.float64).reshape(2, 8)
    date[4] = I64.min        # NaT
    values[:, 5] = np.nan    # all NaN
    values[0, 6] = np.nan    # partly NaN: takes part
    window = (-6 * H, 0, False, True)
    for layout in (COLUMNS, FIELDS):
        winner = check(date, cell, values, target, n_cells, window, 6 * H, 0.0, layout)
        assert winner.tolist() == [[6, 7, -1, -1, -1]]
        winner = check(date[:6], cell[:6], values[:, :6], target, n_cells, window, 6 * H, 0.0, layout)
        assert (winner == -1).all()


def test_two_runs_give_identical_bytes(dev):
    rng = np.random.default_rng(99)
    date, cell, values, targets = random_table(rng, 200_000, 4099, 4, 8)
    runs = [device_run(date, cell, values, targets, 4099, (-9 * H, 3 * H, False, True), 6 * H, 0.3, COLUMNS) for _ in range(2)]
    (s0, w0), (s1, w1) = runs
    assert torch.equal(w0, w1)
    assert torch.equal(s0.data.view(torch.int64), s1.data.view(torch.int64))  # bytes, padding included


def test_contended_cells_keep_the_first_row_among_the_smallest(dev):
    """Every row in 3 cells: hundreds of thousands of atomics per address, and still the lowest row among the smallest scores."""
    rng = np.random.default_rng(5)
    n, n_cells = 300_000, 64
    date, cell, values, targets = random_table(rng, n, n_cells, 2, 4, specials=False)
    cell = rng.choice([3, 17, 63], n).astype(np.int64)
    date = BASE + rng.integers(0, 5 * 360 // 30, n) * 30 * MINUTE  # a 30-minute lattice: thousands of equal scores per cell
    for weight in (0.0, 0.3):
        winner = check(date, cell, values, targets, n_cells, (-6 * H, 0, False, True), 6 * H, weight, FIELDS)
        assert (winner >= 0).sum() == 3 * 4
        for t, c in zip(*np.nonzero(winner >= 0)):
            s = R.scores(date, int(targets[t]), values, 6 * H, weight)
            takes_part = (cell == c) & R.in_window(date, int(targets[t]), (-6 * H, 0, False, True)) & ~np.isnan(values).all(axis=0)
            assert winner[t, c] == np.flatnonzero(takes_part & (s == s[takes_part].min()))[0]


# ---- through the plugin API ------------------------------------------------------------------------------------------------------
@pytest.fixture
def small_grid(monkeypatch):
    lat, lon = np.array(GOLDEN["grid"]["latitudes"]), np.array(GOLDEN["grid"]["longitudes"])
    monkeypatch.setattr(IrregularToGrid, "_define_grid", staticmethod(lambda grid: (lat, lon)))
    return lat, lon


def check_fieldlist(result, table, config, want, lat, lon):
    columns = config["columns"]
    targets = R.unique_in_order(table[config["window_date_column"]].astype("datetime64[ns]").view(np.int64))
    assert len(result) == len(targets) * len(columns) == len(want)
    stacks = {id(f.stack_ref()[0]) for f in result}
    assert len(stacks) <= 1, "the fields of one call are levels of ONE stack"
    for i, field in enumerate(result):  # time-major, then column
        t, j = divmod(i, len(columns))
        assert field.metadata("param") == columns[j]
        valid = field.metadata("valid_datetime")
        assert isinstance(valid, datetime.datetime)
        assert np.datetime64(valid, "ns").astype(np.int64) == targets[t]
        field_lat, field_lon = field.grid_points()
        np.testing.assert_array_equal(field_lat, lat)
        np.testing.assert_array_equal(field_lon, lon)
        assert field.stack_ref() is not None and field.stack_ref()[1] == i
        np.testing.assert_array_equal(field.to_numpy(), want[i])


@pytest.mark.parametrize("case", GOLDEN["reference_cases"], ids=lambda c: c["id"])
def test_filter_reproduces_the_reference_test_cases(dev, small_grid, case):
    lat, lon = small_grid
    table = R.reference_case_table(case)
    result = create_filter_by_name("irregular_to_grid", **case["config"])(table)
    check_fieldlist(result, table, case["config"], R.expected_levels(case, len(lat)), lat, lon)


@pytest.mark.parametrize("case", GOLDEN["random_cases"], ids=lambda c: c["id"])
def test_filter_reproduces_the_recorded_reference_grids(dev, monkeypatch, case):
    n_cells = case["n_cells"]
    lat, lon = np.linspace(-60.0, 60.0, n_cells), np.linspace(0.0, 170.0, n_cells)
    monkeypatch.setattr(IrregularToGrid, "_define_grid", staticmethod(lambda grid: (lat, lon)))
    table = R.random_case_table(case)
    result = create_filter_by_name("irregular_to_grid", **case["config"])(table)
    check_fieldlist(result, table, case["config"], R.expected_levels(case, n_cells), lat, lon)
    # the same table as device tensors (dates as int64 nanoseconds): the same fields
    on_device = {k: torch.from_numpy(v.astype("datetime64[ns]").view(np.int64) if v.dtype.kind == "M" else v).to(dev) for k, v in table.items()}
    again = create_filter_by_name("irregular_to_grid", **case["config"])(on_device)
    check_fieldlist(again, table, case["config"], R.expected_levels(case, n_cells), lat, lon)


def test_filter_takes_a_dataframe(dev, small_grid):
    pd = pytest.importorskip("pandas")
    lat, lon = small_grid
    case = GOLDEN["reference_cases"][0]
    table = R.reference_case_table(case)
    result = create_filter_by_name("irregular_to_grid", **case["config"])(pd.DataFrame(table))
    check_fieldlist(result, table, case["config"], R.expected_levels(case, len(lat)), lat, lon)


def test_regrid_takes_the_output_without_a_host_copy(dev, monkeypatch):
    """``irregular_to_grid | regrid``: the gridded observations are stack-backed, so the regrid gathers from HBM."""
    rng = np.random.default_rng(3)
    n_cells = len(lookup("o32")["latitudes"])
    date, cell, values, targets = random_table(rng, 50_000, n_cells, 2, 2)
    table = {"date": date, "window_date": targets[rng.integers(0, 2, len(date))], "spatial_index": cell, "a": values[0], "b": values[1]}
    gridded = create_filter_by_name("irregular_to_grid", window_date_column="window_date", columns=["a", "b"], grid="o32")
    fields = gridded(table)
    assert all(f.stack_ref() is not None for f in fields)
    from anemoi_transform_amd import fields as fields_module

    def no_host_values(field):
        raise AssertionError("regrid asked for a host copy of a resident field")

    monkeypatch.setattr(fields_module, "host_values", no_host_values)
    pipeline = gridded | create_filter_by_name("regrid", in_grid="o32", out_grid=[5.0, 5.0], method="nearest")
    out = pipeline(table)
    assert len(out) == 4 and all(f.stack_ref() is not None for f in out)
    assert [f.metadata("param") for f in out] == ["a", "b", "a", "b"]
    # nearest neighbour copies values: every regridded value is a value of the gridded field (or NaN where nothing was observed)
    for src, tgt in zip(fields, out):
        got, have = tgt.to_numpy(flatten=True), src.to_numpy(flatten=True)
        assert np.isin(got[~np.isnan(got)], have[~np.isnan(have)]).all() and (~np.isnan(got)).any()


# ---- assign_to_grid --------------------------------------------------------------------------------------------------------------
def test_assign_to_grid_o96_literals(dev):
    case = GOLDEN["assign_to_grid_o96"]
    table = {"latitude": np.array(case["latitude"]), "longitude": np.array(case["longitude"])}
    result = create_filter_by_name("assign_to_grid", grid="o96")(table)
    assert tuple(result) == ("latitude", "longitude", "grid_index_o96", "distance")
    np.testing.assert_array_equal(result["grid_index_o96"], case["grid_index"])
    assert np.allclose(result["distance"], case["distance"])  # the reference's own check
    assert "grid_index_o96" not in table


def test_assign_to_grid_returns_a_dataframe_for_a_dataframe(dev):
    pd = pytest.importorskip("pandas")
    case = GOLDEN["assign_to_grid_o96"]
    df = pd.DataFrame({"latitude": case["latitude"], "longitude": case["longitude"]})
    result = create_filter_by_name("assign_to_grid", grid="o96")(df.copy())
    assert isinstance(result, pd.DataFrame)
    assert tuple(result.columns) == tuple(df.columns) + ("grid_index_o96", "distance")
    np.testing.assert_array_equal(result["grid_index_o96"].to_numpy(), case["grid_index"])


def test_assign_to_grid_equals_ckdtree_on_random_observations(dev):
    from scipy.spatial import cKDTree

    rng = np.random.default_rng(2024)
    n = 200_000
    lat, lon = rng.uniform(-90.0, 90.0, n), rng.uniform(-180.0, 360.0, n)
    grid = lookup("o96")
    grid_lon = np.where(grid["longitudes"] > 180, grid["longitudes"] - 360, grid["longitudes"])
    want_d, want_i = cKDTree(np.column_stack([grid["latitudes"], grid_lon])).query(np.column_stack([lat, lon]))
    result = create_filter_by_name("assign_to_grid", grid="o96")({"latitude": lat, "longitude": lon})
    np.testing.assert_array_equal(result["grid_index_o96"], want_i)
    np.testing.assert_array_equal(result["distance"].view(np.int64), want_d.view(np.int64))  # bit for bit


def test_assign_to_grid_healpix_is_not_implemented(dev):
    with pytest.raises(NotImplementedError, match="healpy"):
        create_filter_by_name("assign_to_grid", grid="h16")({"latitude": np.zeros(1), "longitude": np.zeros(1)})


# ---- full size -------------------------------------------------------------------------------------------------------------------
def test_fullsize_o1280(dev):
    """O1280, 8 targets, 4 columns, 1e7 rows against the vectorised restatement."""
    rng = np.random.default_rng(1280)
    n_cells = len(lookup("o1280")["latitudes"])
    n, n_time, n_cols = 10_000_000, 8, 4
    date = BASE + rng.integers(0, (n_time + 1) * 360, n) * MINUTE
    cell = rng.integers(-3, n_cells + 3, n).astype(np.int64)
    values = rng.integers(0, 1 << 20, (n_cols, n)).astype(np.float64)
    values[rng.random((n_cols, n)) < 0.2] = np.nan
    targets = BASE + np.arange(1, n_time + 1, dtype=np.int64) * 360 * MINUTE
    window = (-9 * H, 0, False, True)
    want, want_winner = R.grid_observations(date, cell, values, targets, n_cells, window, 6 * H, 0.3)
    stack, winner = device_run(date, cell, values, targets, n_cells, window, 6 * H, 0.3, COLUMNS)
    np.testing.assert_array_equal(winner.cpu().numpy(), want_winner)
    got = stack.numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)
    assert 0.05 < (want_winner >= 0).mean() < 0.95
