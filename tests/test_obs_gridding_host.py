"""irregular_to_grid / assign_to_grid without a GPU: registration, errors, the window parser, and the numpy restatement
(tests/obs_gridding_restatement.py) against the golden grids of the reference's own code and against a pandas route written from
the reference's statement (R: filters/tabular/irregular_to_grid.py, tests/tabular_filters/test_irregular_to_grid.py)."""

from __future__ import annotations

import re

import numpy as np
import pytest

import __graft_entry__ as graft
import abi_checks
from anemoi_transform_amd import native, obs
from anemoi_transform_amd.filters import create_filter_by_name, filter_registry
from anemoi_transform_amd.filters.tabular import AssignToGrid, IrregularToGrid

import obs_gridding_restatement as R

GOLDEN = R.load_golden()
H = 3600 * 10**9


def test_the_two_names_are_registered():
    assert filter_registry.is_registered("irregular_to_grid")
    assert filter_registry.is_registered("assign_to_grid")
    f = create_filter_by_name("irregular_to_grid", window_date_column="window_date", columns=["t"])
    assert isinstance(f, IrregularToGrid)
    assert (f.time_freq, f.grid, f.nan_score_weight) == ("6h", "o96", 0.0)  # the reference's defaults
    assert f.window == obs.Window(-6 * H, 0, False, True)  # "(-time_freq, 0]"
    assert isinstance(create_filter_by_name("assign_to_grid", grid="o96"), AssignToGrid)


def test_constructor_errors():
    with pytest.raises(ValueError):
        create_filter_by_name("irregular_to_grid", window_date_column="w", columns=[])
    with pytest.raises(ValueError):
        create_filter_by_name("irregular_to_grid", window_date_column="", columns=["t"])
    for weight in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            create_filter_by_name("irregular_to_grid", window_date_column="w", columns=["t"], nan_score_weight=weight)
    with pytest.raises(ValueError, match="6 hours"):
        create_filter_by_name("irregular_to_grid", window_date_column="w", columns=["t"], window="6 hours")
    with pytest.raises(ValueError):
        create_filter_by_name("assign_to_grid", grid="")
    with pytest.raises(TypeError):
        create_filter_by_name("assign_to_grid")  # keyword-only, required


def test_missing_column_raises_at_forward():
    # R: tests/tabular_filters/test_irregular_to_grid.py:305-321 — before anything touches the device
    f = create_filter_by_name("irregular_to_grid", window_date_column="window_date", time_freq="6h", columns=["temperature", "missing_col"])
    table = {
        "date": np.array(["2023-01-01T05:00"], dtype="datetime64[ns]"),
        "window_date": np.array(["2023-01-01T06:00"], dtype="datetime64[ns]"),
        "spatial_index": np.array([0]),
        "temperature": np.array([10.0]),
    }
    with pytest.raises(ValueError, match="missing_col"):
        f(table)
    with pytest.raises(ValueError, match="longitude"):
        create_filter_by_name("assign_to_grid", grid="o96")({"latitude": np.zeros(2)})


def test_healpix_grids_say_what_is_missing():
    with pytest.raises(NotImplementedError, match="healpy"):
        IrregularToGrid._define_grid("h16")


def test_define_grid_wraps_longitudes():
    lat, lon = IrregularToGrid._define_grid("o96")
    assert len(lat) == len(lon) == 40320
    assert lon.max() <= 180.0 and lon.min() > -180.0


@pytest.mark.parametrize(
    "text, want",
    [
        ("(-6h, 0]", (-6 * H, 0, False, True)),
        ("[-6h, 0]", (-6 * H, 0, True, True)),
        ("(-6h, 0)", (-6 * H, 0, False, False)),
        ("(-3h, +1h]", (-3 * H, 1 * H, False, True)),
        ("[-3h, +3h)", (-3 * H, 3 * H, True, False)),
        ("(-6h, 0h]", (-6 * H, 0, False, True)),
        ("[-90m,30s]", (-90 * 60 * 10**9, 30 * 10**9, True, True)),
        ("(-1d, 0]", (-24 * H, 0, False, True)),
    ],
)
def test_window_parser(text, want):
    assert tuple(obs.parse_window(text)) == want


@pytest.mark.parametrize("text", ["", "-6h, 0", "(-6h 0]", "(-6x, 0]", "(-6h, 0, 1h]", "(6h, 0]", "{-6h, 0}", "(-1.5h, 0]"])
def test_window_parser_names_the_string(text):
    with pytest.raises(ValueError, match=re.escape(repr(text))):
        obs.parse_window(text)


def test_frequency_and_date_conversion():
    assert obs.parse_frequency("6h") == 6 * H and obs.parse_frequency("30m") == H // 2 and obs.parse_frequency("1d") == 24 * H
    for bad in ("0h", "six", "-6h"):
        with pytest.raises(ValueError):
            obs.parse_frequency(bad)
    seconds = np.array(["2023-01-01T06:00:00", "NaT"], dtype="datetime64[s]")
    ns = obs.to_ns(seconds)
    assert ns.dtype == np.int64 and ns[0] == 1672552800 * 10**9 and ns[1] == obs.NAT
    assert list(obs.unique_in_order(np.array([7, 3, 7, 1, 3], dtype=np.int64))) == [7, 3, 1]
    assert list(obs.to_cells(np.array([2.0, np.nan, 5.0]))) == [2, -1, 5]
    with pytest.raises(ValueError):
        obs.to_cells(np.array([2.5]))
    with pytest.raises(ValueError):
        obs.to_values([np.array(["a", "b"])])


# ---- the restatement against the reference ---------------------------------------------------------------------------------------
def _run(table, config, n_cells):
    return R.run_table(table, config, n_cells, obs.parse_window, obs.parse_frequency)


@pytest.mark.parametrize("case", GOLDEN["reference_cases"], ids=lambda c: c["id"])
def test_restatement_reproduces_the_reference_test_cases(case):
    n_cells = len(GOLDEN["grid"]["latitudes"])
    np.testing.assert_array_equal(_run(R.reference_case_table(case), case["config"], n_cells), R.expected_levels(case, n_cells))


@pytest.mark.parametrize("case", GOLDEN["random_cases"], ids=lambda c: c["id"])
def test_restatement_reproduces_the_recorded_reference_grids(case):
    want = R.expected_levels(case, case["n_cells"])
    assert np.isfinite(want).sum() > 300, "a golden table that fills nothing tests nothing"
    np.testing.assert_array_equal(_run(R.random_case_table(case), case["config"], case["n_cells"]), want)


def test_golden_has_the_cases_it_should():
    assert len(GOLDEN["reference_cases"]) == 6 and len(GOLDEN["random_cases"]) >= 3
    assert sorted(c["config"]["nan_score_weight"] for c in GOLDEN["random_cases"])[:3] == [0.0, 0.3, 1.0]


def _pandas_route(pd, df, columns, targets, window, freq, weight, n_cells):
    """The reference's statement, written out with pandas (one process, a loop over targets with a groupby in each)."""
    before, after, closed_before, closed_after = window
    grids = {c: np.full((len(targets), n_cells), np.nan) for c in columns}
    for t, target in enumerate(targets):
        lo, hi = target + pd.Timedelta(before, "ns"), target + pd.Timedelta(after, "ns")
        mask = (df["date"].ge(lo) if closed_before else df["date"].gt(lo)) & (df["date"].le(hi) if closed_after else df["date"].lt(hi))
        part = df[mask]
        part = part[~part[columns].isna().all(axis=1)].copy()
        if len(part) == 0:
            continue
        score = (part["date"] - target).abs() / freq
        if weight > 0:
            score = (1.0 - weight) * score + weight * (part[columns].isna().sum(axis=1) / len(columns))
        part["_score"] = score
        best = part.loc[part.groupby("spatial_index")["_score"].idxmin()]
        index = best["spatial_index"].values.astype(np.intp)
        ok = (index >= 0) & (index < n_cells)
        for c in columns:
            grids[c][t, index[ok]] = best[c].values[ok]
    return np.stack([grids[c][t] for t in range(len(targets)) for c in columns]) if len(targets) else np.zeros((0, n_cells))


@pytest.mark.parametrize("seed", range(20))
def test_restatement_equals_a_pandas_route(seed):
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(1000 + seed)
    n, n_cells = int(rng.integers(50, 1500)), int(rng.integers(3, 80))
    columns = [f"v{j}" for j in range(int(rng.integers(1, 5)))]
    window_text = ["(-6h, 0]", "[-6h, 0]", "(-9h, +3h)", "[-3h, +3h)", "(-12h, +1h]"][seed % 5]
    weight = [0.0, 0.3, 1.0, 0.05][seed % 4]
    base = np.datetime64("2024-02-28T00:00", "ns")
    minute = np.timedelta64(60 * 10**9, "ns")
    lattice = int(rng.choice([1, 10, 30]))
    table = {
        "date": base + rng.integers(0, 48 * 60 // lattice, n) * lattice * minute,
        "window_date": base + rng.integers(1, 8, n) * 360 * minute,
        "spatial_index": rng.integers(-2, n_cells + 2, n),
    }
    table["date"][rng.integers(0, n, 3)] = np.datetime64("NaT")
    for c in columns:
        v = rng.integers(0, 50, n).astype(np.float64)
        v[rng.random(n) < 0.3] = np.nan
        table[c] = v
    config = {"window_date_column": "window_date", "columns": columns, "window": window_text, "nan_score_weight": weight, "time_freq": "6h"}
    df = pd.DataFrame(table)
    targets = pd.to_datetime(df["window_date"].unique())
    want = _pandas_route(pd, df, columns, targets, tuple(obs.parse_window(window_text)), pd.Timedelta("6h"), weight, n_cells)
    got = _run(table, config, n_cells)
    assert np.isfinite(want).any()
    np.testing.assert_array_equal(got, want)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    names = ("atx_obs_best_per_cell", "atx_obs_fill_stack")
    declared = graft.exported_names()
    exported, _ = abi_checks.defined_dynamic_symbols(graft.LIB)
    for name in names:
        assert name in declared, f"{name} is not declared in include/atx.h"
        assert name in native.SIGNATURES, f"{name} is not bound in native.py"
        assert name in exported, f"{name} is not exported by libatx.so"
    assert native.load().atx_version() == 420


def test_abi_argument_validation_without_a_gpu():
    lib = native.load()

    def call(n_obs=0, n_cols=1, pitch=0, n_time=0, n_cells=4, freq=6 * H, w=0.0):
        return lib.atx_obs_best_per_cell(None, None, None, n_obs, n_cols, pitch, None, n_time, n_cells, -6 * H, 0, 0, 1, freq, w, None, None, None)

    assert call() == native.OK  # no targets: nothing to do, nothing dereferenced
    assert call(n_obs=2**31, pitch=2**31) == native.EINVAL
    assert b"int32" in lib.atx_last_error()
    assert call(freq=0) == native.EINVAL
    assert call(w=1.5) == native.EINVAL
    assert call(n_cols=0) == native.EINVAL
    assert lib.atx_obs_fill_stack(None, None, 0, 1, 0, 0, 4, None, 4, native.FIELDS, None) == native.OK
    assert lib.atx_obs_fill_stack(None, None, 0, 1, 0, 0, 4, None, 4, 7, None) == native.EINVAL
    assert lib.atx_obs_fill_stack(None, None, 2**31, 1, 2**31, 1, 4, None, 4, native.FIELDS, None) == native.EINVAL
