"""``irregular_to_grid`` restated in numpy, without pandas — TEST INFRASTRUCTURE (``oracle/`` is frozen, so the statement lives here).

R: filters/tabular/irregular_to_grid.py — per target ``t`` (``forward`` :139-159):
  select_window   :209-254  rows with  t + before <(=) date <(=) t + after  whose columns are not ALL NaN
  get_nearest_obs :256-317  score = |date - t| / time_freq  (w > 0: (1.0 - w) * that + w * (nan_count / len(columns))),
                            ``groupby("spatial_index").idxmin()``: per cell the row of smallest score, the first row of the
                            table among equal scores
  _fill_grids     :190-207  winners with 0 <= spatial_index < n_grid write their values at [t, spatial_index] of NaN grids
restated POSITIONALLY: rows are numbered 0 .. n_obs - 1 in table order and "first" is the smallest number.  tests/golden/
irregular_to_grid.json holds grids the reference's own three functions produced for seeded tables (tools/
record_irregular_to_grid_golden.py); tests/test_obs_gridding_host.py holds this file to them with assert_array_equal.

Vectorised per target: one lexsort on (cell, score, row) and the first row of every run of equal cells, so that the full-size case
(1e7 rows onto O1280) is affordable.  Dates and targets are int64 nanoseconds, NaT = INT64_MIN.
"""

from __future__ import annotations

import json
import os

import numpy as np

NAT = np.iinfo(np.int64).min
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "irregular_to_grid.json")


def scores(date_ns, target_ns: int, values, freq_ns: int, weight: float) -> np.ndarray:
    """The selection score of every row for one target (float64 ``[n_obs]``): int64 ns -> float64, one division."""
    time_score = np.abs(date_ns - np.int64(target_ns)).astype(np.float64) / np.float64(freq_ns)
    if weight > 0:
        nan_score = np.isnan(values).sum(axis=0) / values.shape[0]
        return (1.0 - weight) * time_score + weight * nan_score
    return time_score


def in_window(date_ns, target_ns: int, window) -> np.ndarray:
    before_ns, after_ns, closed_before, closed_after = window
    if target_ns == NAT:
        return np.zeros(len(date_ns), dtype=bool)
    lo, hi = np.int64(target_ns) + np.int64(before_ns), np.int64(target_ns) + np.int64(after_ns)
    mask = (date_ns >= lo) if closed_before else (date_ns > lo)
    mask &= (date_ns <= hi) if closed_after else (date_ns < hi)
    return mask & (date_ns != NAT)


def best_per_cell(date_ns, cell, values, target_ns, n_cells: int, window, freq_ns: int, weight: float) -> np.ndarray:
    """``winner[t, c]`` (int32): the row target ``t`` shows in cell ``c``, -1 for none.  ``values`` is ``[n_cols, n_obs]``;
    ``window`` is ``(before_ns, after_ns, closed_before, closed_after)``."""
    date_ns, cell = np.asarray(date_ns, dtype=np.int64), np.asarray(cell, dtype=np.int64)
    values = np.asarray(values, dtype=np.float64).reshape(len(values), -1)
    winner = np.full((len(target_ns), n_cells), -1, dtype=np.int32)
    usable = ~np.isnan(values).all(axis=0) & (cell >= 0) & (cell < n_cells)
    for t, target in enumerate(np.asarray(target_ns, dtype=np.int64)):
        rows = np.nonzero(usable & in_window(date_ns, int(target), window))[0]
        if rows.size == 0:
            continue
        s = scores(date_ns[rows], int(target), values[:, rows], freq_ns, weight)
        order = np.lexsort((rows, s, cell[rows]))  # by cell, then score, then row
        c = cell[rows][order]
        first = np.ones(len(c), dtype=bool)
        first[1:] = c[1:] != c[:-1]
        winner[t, c[first]] = rows[order][first]
    return winner


def fill(winner, values) -> np.ndarray:
    """``[n_time * n_cols, n_cells]`` float64: level ``t * n_cols + j`` is ``values[j, winner[t]]``, NaN where the winner is -1."""
    values = np.asarray(values, dtype=np.float64).reshape(len(values), -1)
    n_time, n_cells = winner.shape
    out = np.full((n_time, values.shape[0], n_cells), np.nan)
    t, c = np.nonzero(winner >= 0)
    out[t, :, c] = values[:, winner[t, c]].T
    return out.reshape(n_time * values.shape[0], n_cells)


def unique_in_order(x) -> np.ndarray:
    """``Series.unique()``: distinct values in order of first appearance."""
    uniq, first = np.unique(np.asarray(x), return_index=True)
    return uniq[np.argsort(first, kind="stable")]


def grid_observations(date_ns, cell, values, target_ns, n_cells, window, freq_ns, weight):
    """``(stack [n_time * n_cols, n_cells], winner)``."""
    winner = best_per_cell(date_ns, cell, values, target_ns, n_cells, window, freq_ns, weight)
    return fill(winner, values), winner


# ---- the golden file -----------------------------------------------------------------------------------------------------------
def load_golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


def _floats(xs) -> np.ndarray:
    return np.array([np.nan if x is None else x for x in xs], dtype=np.float64)


def reference_case_table(case: dict) -> dict[str, np.ndarray]:
    """A transcribed case of the reference's test as a mapping of numpy columns (dates as datetime64[ns])."""
    table = {}
    for name, column in case["table"].items():
        if name in ("date", "window_date"):
            table[name] = np.array(column, dtype="datetime64[ns]")
        elif name == "spatial_index":
            table[name] = np.array(column, dtype=np.int64)
        else:
            table[name] = _floats(column)
    return table


def expected_levels(case: dict, n_cells: int) -> np.ndarray:
    """The expected grids of a golden case as the stack ``[n_time * n_cols, n_cells]``, time-major then column."""
    columns = case["config"]["columns"]
    n_time = len(case["expected"][columns[0]])
    out = np.full((n_time * len(columns), n_cells), np.nan)
    for j, name in enumerate(columns):
        for t, row in enumerate(case["expected"][name]):
            out[t * len(columns) + j] = _floats(row)
    return out


def random_case_table(case: dict) -> dict[str, np.ndarray]:
    """A recorded random case as a mapping of numpy columns.  The file stores, per row, the date and the window date in steps
    of ``date_step_min`` / ``window_step_min`` whole minutes after ``base``, the cell and a bit mask of the columns that are NaN; the value of column ``j`` in row ``r`` is the whole
    number ``r * n_cols + j``, so that a grid names the row it was filled from."""
    base = np.datetime64(case["base"], "ns")
    minute = np.timedelta64(60 * 10**9, "ns")
    columns = case["config"]["columns"]
    n = len(case["date_step"])
    table = {
        "date": base + np.array(case["date_step"], dtype=np.int64) * case["date_step_min"] * minute,
        "window_date": base + np.array(case["window_step"], dtype=np.int64) * case["window_step_min"] * minute,
        "spatial_index": np.array(case["cell"], dtype=np.int64),
    }
    nat = np.array(case.get("nat_rows", []), dtype=np.int64)
    table["date"][nat] = np.datetime64("NaT")
    mask = np.array(case["nan_mask"], dtype=np.int64)
    for j, name in enumerate(columns):
        v = (np.arange(n, dtype=np.float64) * len(columns) + j)
        v[(mask >> j) & 1 == 1] = np.nan
        table[name] = v
    return table


def run_table(table: dict, config: dict, n_cells: int, parse_window, parse_frequency) -> np.ndarray:
    """The restatement on a table of numpy columns with the filter's configuration -> ``[n_time * n_cols, n_cells]``."""
    freq_ns = parse_frequency(config.get("time_freq", "6h"))
    window = tuple(parse_window(config.get("window") or f"(-{config.get('time_freq', '6h')}, 0]"))
    date_ns = table["date"].astype("datetime64[ns]").view(np.int64)
    targets = unique_in_order(table[config["window_date_column"]].astype("datetime64[ns]").view(np.int64))
    values = np.stack([np.asarray(table[c], dtype=np.float64) for c in config["columns"]]).reshape(len(config["columns"]), -1)
    stack, _ = grid_observations(date_ns, table["spatial_index"], values, targets, n_cells, window, freq_ns,
                                 float(config.get("nan_score_weight", 0.0)))
    return stack
