"""Missing station altitudes from an orography on the device: ``atx_obs_fill_heights`` (csrc/atx_obs_fill_heights.hip) through
``obs.fill_heights`` and the ``fill_orography`` filter, and ``geopotential_to_height_tabular`` on device tensors, held against the
reference's literals and recorded frames (tests/golden/fill_heights.json) and the numpy / scipy restatement
(tests/fill_heights_restatement.py).

The kernel decides every row whose nearest axis entry is strictly the nearest; there its answer must equal the restatement's bit for
bit (compared as int64, so -0.0 and NaN payloads count).  No seeded row is a tie (test_fill_heights_host.py checks that without a
GPU), so for the seeded rows the flagged counter must be 0.  Rows that ARE ties must be flagged with the right bit per axis and come
back, through the host's cKDTree, with the reference's recorded answers.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import fill_heights_restatement as R
from anemoi_transform_amd import native, obs
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.filters.tabular import FillHeights

pytestmark = pytest.mark.gpu

CASES = R.load_golden()
BY_ID = {case["id"]: case for case in CASES}
TABLE = R.rows(max(R.ROWS))  # the largest launch; a launch of n rows takes the first n
_GRIDS: dict = {}


def _dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t) -> np.ndarray:
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float64
    return np.ascontiguousarray(a).view(np.int64)


def _launch(grid: obs.HeightGrid, latitude, longitude, altitude):
    """``(out, flags, counters)`` of one call of the entry point, as host arrays."""
    n = len(altitude)
    out = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    flags = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    counters = torch.full((3,), 99, dtype=torch.int64, device="cuda")  # the call sets them, whatever they held
    native.obs_fill_heights(_dev(latitude), _dev(longitude), _dev(altitude), grid.d_sorted[0], grid.d_order[0], grid.d_sorted[1],
                            grid.d_order[1], grid.heights, out, flags, counters)
    return out.cpu().numpy(), flags.cpu().numpy(), counters.cpu().numpy().tolist()


def _seeded(shape, kind, dtype):
    """``(grid in HBM, the restatement's column for the largest launch)``, once per process.  float64 heights sit in a wider block:
    their pitch is larger than ``n_lon``."""
    key = (shape, kind, np.dtype(dtype).name)
    if key not in _GRIDS:
        lat_axis, lon_axis = R.axes(kind, *shape)
        h = R.heights(*shape, dtype)
        want = R.fill(lat_axis, lon_axis, h, TABLE["latitude"], TABLE["longitude"], TABLE["stalt"])
        if dtype == np.float64:
            block = torch.full((shape[0], shape[1] + 5), -1.0, dtype=torch.float64, device="cuda")
            block[:, :shape[1]] = _dev(h)
            resident = block[:, :shape[1]]
            assert resident.stride(0) == shape[1] + 5
        else:
            resident = h
        _GRIDS[key] = (obs.HeightGrid(lat_axis, lon_axis, resident), want)
    return _GRIDS[key]


# ---- the reference's literals ----------------------------------------------------------------------------------------------------------
def _patched_filter(monkeypatch, case, calls):
    config = case["config"]
    names = (config.get("orography_altitude", "z"), config.get("orography_latitude", "latitude"), config.get("orography_longitude", "longitude"))

    def open_orography(path, altitude, latitude, longitude):
        assert path == config["orography_file"] and (altitude, latitude, longitude) == names
        calls.append(path)
        return case["lat_axis"], case["lon_axis"], case["heights"]

    monkeypatch.setattr(FillHeights, "_open_orography", staticmethod(open_orography))
    return create_filter_by_name("fill_orography", **config)


LITERAL_IDS = [case["id"] for case in CASES if "literals" in case]


@pytest.mark.parametrize("case_id", LITERAL_IDS)
def test_filter_gives_the_reference_literals_on_every_kind_of_table(monkeypatch, case_id):
    pd = pytest.importorskip("pandas")
    case, calls = BY_ID[case_id], []
    column, table = case["column"], case["table"]
    f = _patched_filter(monkeypatch, case, calls)

    df = pd.DataFrame(table)
    before = df.copy()
    out = f(df)
    assert isinstance(out, pd.DataFrame) and tuple(out.columns) == tuple(df.columns) and out.shape == df.shape
    assert out[["latitude", "longitude"]].equals(df[["latitude", "longitude"]])
    assert out[column].tolist() == [1.0, 2.0, 3.0, 4.0] and out[column].dtype == np.float64
    assert df.equals(before) and out is not df  # the caller's table is as it was

    host = {name: col.copy() for name, col in table.items()}
    out = f(host)
    assert isinstance(out, dict) and list(out) == list(table) and isinstance(out[column], np.ndarray) and out is not host
    assert out[column].tolist() == [1.0, 2.0, 3.0, 4.0] and out["latitude"] is host["latitude"]
    assert all(R.same_bits(host[name], table[name]) for name in table)

    resident = {name: _dev(col) for name, col in table.items()}
    out = f(resident)
    assert list(out) == list(table) and all(isinstance(v, torch.Tensor) and v.is_cuda for v in out.values())
    assert out[column].dtype == torch.float64 and out[column].cpu().tolist() == [1.0, 2.0, 3.0, 4.0]
    assert out["latitude"] is resident["latitude"] and out[column] is not resident[column]
    assert all(R.same_bits(resident[name].cpu().numpy(), table[name]) for name in table)
    assert calls == [case["config"]["orography_file"]]  # opened once per instance, on first use


def test_filter_without_the_altitude_column_raises(monkeypatch):
    case, calls = BY_ID["reference_test_fill_heights_missing_station_altitude"], []
    f = _patched_filter(monkeypatch, case, calls)
    with pytest.raises(ValueError, match=r"missing columns: \{'stalt'\}"):
        f({name: _dev(col) for name, col in case["table"].items()})
    assert calls == []


@pytest.mark.parametrize("case_id", [case["id"] for case in CASES if case["id"].startswith("seeded_")])
def test_filter_equals_the_recorded_frames(monkeypatch, case_id):
    case = BY_ID[case_id]
    out = _patched_filter(monkeypatch, case, [])({name: _dev(col) for name, col in case["table"].items()})
    assert np.array_equal(_bits(out["stalt"]), _bits(case["expected"]))


# ---- seeded rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ROWS)
def test_seeded_rows_equal_the_restatement_bit_for_bit(n):
    lat, lon, alt = (TABLE[name][:n] for name in ("latitude", "longitude", "stalt"))
    n_fill = int(R.to_fill(alt).sum())
    for shape in R.SHAPES:
        for kind in R.KINDS:
            for dtype in (np.float32, np.float64):
                grid, want = _seeded(shape, kind, dtype)
                what = f"n={n} {shape} {kind} {np.dtype(dtype).name}"
                out, flags, (filled, flagged, bad) = _launch(grid, lat, lon, alt)
                print(f"{what}: filled {filled} (restatement {n_fill}), flagged {flagged}, not finite {bad}")
                assert np.array_equal(_bits(out), _bits(want[:n])), what
                assert (filled, flagged, bad) == (n_fill, 0, 0) and not flags.any(), what
                got, counts = obs.fill_heights(grid, _dev(lat), _dev(lon), _dev(alt), return_counts=True)
                assert got.is_cuda and got.dtype == torch.float64 and got.shape == (n,) and counts == (n_fill, 0)
                assert np.array_equal(_bits(got), _bits(want[:n])), what


def test_rows_past_the_grid_cap():
    """The launch is capped at 2048 workgroups of 256 lanes (kFhGrid): from 524 288 rows on a lane takes more than one row."""
    n = 2048 * 256 + 300
    table = R.rows(n, seed=77)
    lat_axis, lon_axis = R.axes("shuffled", 181, 360)
    h = R.heights(181, 360, np.float32)
    grid = obs.HeightGrid(lat_axis, lon_axis, h)
    want = R.fill(lat_axis, lon_axis, h, table["latitude"], table["longitude"], table["stalt"])
    want_bits = R.tie_bits(lat_axis, lon_axis, table["latitude"], table["longitude"], table["stalt"])
    out, flags, (filled, flagged, bad) = _launch(grid, table["latitude"], table["longitude"], table["stalt"])
    strict = want_bits == 0
    print(f"n={n}: filled {filled}, flagged {flagged} (restatement {int((~strict).sum())})")
    assert np.array_equal(flags, want_bits) and (filled, flagged, bad) == (int(R.to_fill(table["stalt"]).sum()), int((~strict).sum()), 0)
    assert np.array_equal(_bits(out)[strict], _bits(want)[strict])
    got = obs.fill_heights(grid, table["latitude"], table["longitude"], table["stalt"])
    assert np.array_equal(_bits(got), _bits(want))


# ---- ties ------------------------------------------------------------------------------------------------------------------------------
def test_midpoint_rows_are_flagged_and_come_back_as_recorded():
    case = BY_ID["midpoints"]
    table = case["table"]
    grid = obs.HeightGrid(case["lat_axis"], case["lon_axis"], case["heights"])
    n = len(table["stalt"])
    _, flags, (filled, flagged, bad) = _launch(grid, table["latitude"], table["longitude"], table["stalt"])
    assert (filled, flagged, bad) == (n, n, 0)
    want_bits = R.tie_bits(case["lat_axis"], case["lon_axis"], table["latitude"], table["longitude"], table["stalt"])
    assert np.array_equal(flags, want_bits) and set(flags.tolist()) == {1, 2, 3}
    assert grid._trees == [None, None]  # the launch alone builds no tree
    got, counts = obs.fill_heights(grid, table["latitude"], table["longitude"], table["stalt"], return_counts=True)
    assert counts == (n, n) and np.array_equal(_bits(got), _bits(case["expected"]))
    assert all(tree is not None for tree in grid._trees)
    trees = list(grid._trees)
    obs.fill_heights(grid, table["latitude"], table["longitude"], table["stalt"])
    assert grid._trees[0] is trees[0] and grid._trees[1] is trees[1]  # built once per grid


def test_no_tree_is_built_without_a_tie():
    grid, want = _seeded((181, 360), "shuffled", np.float32)
    grid._trees = [None, None]
    got = obs.fill_heights(grid, TABLE["latitude"], TABLE["longitude"], TABLE["stalt"])
    assert np.array_equal(_bits(got), _bits(want)) and grid._trees == [None, None]


def test_squares_that_underflow_or_round_to_equal_values_are_flagged():
    lat_axis, lon_axis = np.arange(-2, 3) * 1e-170, np.array([0.0, 10.0])
    h = R.heights(5, 2, np.float64)
    grid = obs.HeightGrid(lat_axis, lon_axis, h)
    lat = np.array([1e-171, 0.0, 1.0, -3e-170, 1e-171])
    lon = np.array([1.0, 9.0, 1.0, 2.0, 5.0])  # the last one: an exact midpoint in longitude as well
    alt = np.full(5, np.nan)
    assert R.ties(lat_axis, lat).all() and R.ties(lon_axis, lon).tolist() == [False] * 4 + [True]
    _, flags, (filled, flagged, bad) = _launch(grid, lat, lon, alt)
    assert flags.tolist() == [1, 1, 1, 1, 3] and (filled, flagged, bad) == (5, 5, 0)
    got = obs.fill_heights(grid, lat, lon, alt)
    assert np.array_equal(_bits(got), _bits(R.fill(lat_axis, lon_axis, h, lat, lon, alt)))  # cKDTree's own answers


# ---- kept rows, rows that cannot be answered -----------------------------------------------------------------------------------------
def test_kept_rows_pass_through_bit_for_bit():
    grid, _ = _seeded((2, 3), "ascending", np.float32)
    alt = np.array([np.inf, -np.inf, -0.0, 0.0, 5e-324, -2.2250738585072014e-308, 9998.999999999998, 9999.000000000002, -9999.0, 1e308])
    assert not R.to_fill(alt).any()
    lat = np.array([np.nan, np.inf, -np.inf, 1e300, 0.0] * 2)  # kept rows may hold anything here
    lon = lat[::-1].copy()
    out, flags, counters = _launch(grid, lat, lon, alt)
    assert np.array_equal(_bits(out), _bits(alt)) and not flags.any() and counters == [0, 0, 0]
    got = obs.fill_heights(grid, lat, lon, alt)
    assert np.array_equal(_bits(got), _bits(alt))


def test_rows_to_fill_without_finite_coordinates_raise(monkeypatch):
    grid, _ = _seeded((181, 360), "descending", np.float32)
    lat_axis, lon_axis = R.axes("descending", 181, 360)
    table = {name: col[:257].copy() for name, col in TABLE.items()}
    bad = [3, 64, 130, 256]
    table["stalt"][bad] = [np.nan, R.SENTINEL, np.nan, R.SENTINEL]
    table["latitude"][3], table["longitude"][64], table["latitude"][130], table["longitude"][256] = np.nan, np.inf, -np.inf, np.nan
    kept = np.flatnonzero(~R.to_fill(table["stalt"]))[:2]
    table["latitude"][kept[0]], table["longitude"][kept[1]] = np.nan, np.inf  # kept rows with such coordinates are harmless
    n_fill = int(R.to_fill(table["stalt"]).sum())
    with pytest.raises(ValueError, match=rf"\b4 of {n_fill} rows to fill"):
        obs.fill_heights(grid, table["latitude"], table["longitude"], table["stalt"])
    monkeypatch.setattr(FillHeights, "_open_orography", staticmethod(lambda *a: (lat_axis, lon_axis, R.heights(181, 360, np.float32))))
    with pytest.raises(ValueError, match=rf"\b4 of {n_fill} rows to fill"):
        create_filter_by_name("fill_orography", orography_file="orography.npz")(table)
    out, flags, (filled, flagged, n_bad) = _launch(grid, table["latitude"], table["longitude"], table["stalt"])
    assert (filled, flagged, n_bad) == (n_fill - 4, 0, 4) and np.isnan(out[bad]).all() and not flags.any()
    good = np.setdiff1d(np.arange(257), bad)
    want = R.fill(lat_axis, lon_axis, R.heights(181, 360, np.float32), table["latitude"][good], table["longitude"][good], table["stalt"][good])
    assert np.array_equal(_bits(out[good]), _bits(want))


def test_nothing_to_fill_and_an_empty_table(monkeypatch):
    grid, _ = _seeded((2, 3), "shuffled", np.float64)
    alt = np.arange(300.0)
    got, counts = obs.fill_heights(grid, np.zeros(300), np.zeros(300), alt, return_counts=True)
    assert counts == (0, 0) and np.array_equal(_bits(got), _bits(alt))
    empty = np.zeros(0)
    got, counts = obs.fill_heights(grid, empty, empty, empty, return_counts=True)
    assert got.shape == (0,) and got.dtype == torch.float64 and got.is_cuda and counts == (0, 0)
    lat_axis, lon_axis = R.axes("shuffled", 2, 3)
    monkeypatch.setattr(FillHeights, "_open_orography", staticmethod(lambda *a: (lat_axis, lon_axis, R.heights(2, 3, np.float64))))
    out = create_filter_by_name("fill_orography", orography_file="orography.npz")({"latitude": empty, "longitude": empty, "stalt": empty})
    assert isinstance(out["stalt"], np.ndarray) and out["stalt"].shape == (0,) and out["stalt"].dtype == np.float64
    with pytest.raises(ValueError, match="differ in length"):
        obs.fill_heights(grid, np.zeros(3), np.zeros(2), np.zeros(3))


# ---- column kinds ----------------------------------------------------------------------------------------------------------------------
def test_strided_and_float32_columns_equal_their_float64_copies():
    grid, want = _seeded((181, 360), "ascending", np.float32)
    block = _dev(np.stack([TABLE["latitude"], TABLE["longitude"], TABLE["stalt"]], axis=1))  # [n, 3]: every column has stride 3
    assert not block[:, 2].is_contiguous()
    got = obs.fill_heights(grid, block[:, 0], block[:, 1], block[:, 2])
    assert np.array_equal(_bits(got), _bits(want))
    cols32 = [_dev(TABLE[name].astype(np.float32)) for name in ("latitude", "longitude", "stalt")]
    got32 = obs.fill_heights(grid, *cols32)
    assert torch.equal(got32.view(torch.int64), obs.fill_heights(grid, *[c.double().contiguous() for c in cols32]).view(torch.int64))
    assert got32.dtype == torch.float64


def test_an_index_into_the_heights_past_2_to_the_31():
    """Row 1 of a two-row orography starts 2^31 + 8 elements after row 0: ``i * pitch + j`` does not fit 32 bits."""
    pitch, n_lon = 2**31 + 8, 8
    flat = torch.empty(pitch + n_lon, dtype=torch.float32, device="cuda")
    h = torch.as_strided(flat, (2, n_lon), (pitch, 1))
    values = np.arange(16, dtype=np.float32).reshape(2, n_lon) + 0.5
    h.copy_(_dev(values))
    lat_axis, lon_axis = np.array([-45.0, 45.0]), np.arange(n_lon) * 45.0
    grid = obs.HeightGrid(lat_axis, lon_axis, h)
    lat, lon = np.array([-50.0, 44.0, 60.0, 1.0]), np.array([0.0, 100.0, 330.0, 46.0])
    alt = np.array([np.nan, R.SENTINEL, np.nan, 7.0])
    got = obs.fill_heights(grid, lat, lon, alt)
    assert np.array_equal(_bits(got), _bits(R.fill(lat_axis, lon_axis, values, lat, lon, alt)))
    assert got.cpu().tolist() == [0.5, 10.5, 15.5, 7.0]
    del grid, h, flat
    torch.cuda.empty_cache()  # 8.6 GB of address range, of which a few pages were touched


# ---- geopotential_to_height on device tensors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["geopotential_to_height", "geopotential_to_height_tabular"])
def test_geopotential_to_height_on_device_tensors_has_numpys_bits(name):
    rng = np.random.default_rng(5)
    z = np.concatenate([rng.uniform(-5e3, 9e5, 4099), rng.standard_normal(500) * 10.0 ** rng.integers(-300, 300, 500),
                        [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 9.80665, 1.7976931348623157e308]])
    table = {"z": _dev(z), "other": _dev(np.arange(z.size))}
    out = create_filter_by_name(name, geopotential="z", height="h")(table)
    assert list(out) == ["z", "other", "h"] and out["h"].is_cuda and out["h"].dtype == torch.float64 and out["z"] is table["z"]
    assert np.array_equal(_bits(out["h"]), _bits(z / 9.80665))
    assert np.array_equal(_bits(table["z"]), _bits(z)) and "h" not in table
    z32 = _dev(z[:4099].astype(np.float32))
    out = create_filter_by_name(name, geopotential="z", height="z")({"z": z32})
    assert out["z"].dtype == torch.float64 and np.array_equal(_bits(out["z"]), _bits(z[:4099].astype(np.float32).astype(np.float64) / 9.80665))
