"""superob in plain numpy with a scalar Kahan loop, independent of the package (R: filters/tabular/superob.py:60-97,
support/superob.py:43-69).  Helper of test_superob_host.py / test_gpu_superob.py; holds no tests.

The statement, for a table (a dict ``name -> 1-D array``) with ``date``, ``latitude``, ``longitude`` and other columns:
  1. rows where ``date``, ``latitude`` or ``longitude`` is missing are dropped;
  2. ``spatial_index``, ``distance``: the nearest grid point in the plane of (latitude, longitude) degrees (cKDTree);
  3. ``temporal = (date - min(date)) // (timeslot_length * 1e9 ns)``, ``grid_index = spatial_index + n_grid * temporal``;
  4. groups by ``(grid_index, *groupby)`` in order of first appearance, rows with a missing key entry dropped;
  5. per group every other column not in ``nearest`` gets pandas' group mean — ONE Kahan sum in row order, missing values skipped,
     ``sum / count``; int columns summed as float64; datetimes summed as float64 nanoseconds, the quotient truncated to int64 —
     and every column in ``nearest`` the value of the first row of smallest ``distance``;
  6. ``grid_index`` and ``distance`` are dropped, columns ordered ``groupby``, averaged (table order), ``nearest``;
  7. rows sorted by ``date``, stably (NaT last).
"""

from __future__ import annotations

import json
import os

import numpy as np

NAT = np.iinfo(np.int64).min
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "superob.json")


def kahan_mean(values) -> tuple[float, int]:
    """pandas/_libs/groupby.pyx group_mean for one group and column: ``(sum / count, count)``, NaN for count 0."""
    total = comp = 0.0
    count = 0
    for v in np.asarray(values, dtype=np.float64).tolist():
        if v != v:
            continue
        y = v - comp
        t = total + y
        comp = (t - total) - y
        if comp != comp:
            comp = 0.0
        total = t
        count += 1
    if count == 0:
        return float("nan"), 0
    with np.errstate(all="ignore"):
        return float(np.float64(total) / np.float64(count)), count


def kahan_means_of_many(groups: list[np.ndarray]) -> np.ndarray:
    """The same loop over MANY groups at once: step k of every group in one numpy statement (same operations, same order within a
    group, so the same bits).  For the sampled groups of a large table."""
    if not groups:
        return np.zeros(0)
    longest = max(len(g) for g in groups)
    padded = np.full((len(groups), longest), np.nan)
    for i, g in enumerate(groups):
        padded[i, : len(g)] = g
    total, comp, count = np.zeros(len(groups)), np.zeros(len(groups)), np.zeros(len(groups), dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(longest):
            v = padded[:, k]
            ok = ~np.isnan(v)
            y = v - comp
            t = total + y
            c = (t - total) - y
            c = np.where(np.isnan(c), 0.0, c)
            total, comp, count = np.where(ok, t, total), np.where(ok, c, comp), count + ok
        return np.where(count > 0, total / np.where(count > 0, count, 1), np.nan)


def is_missing(column: np.ndarray) -> np.ndarray:
    a = np.asarray(column)
    if a.dtype.kind == "M":
        return np.isnat(a)
    if a.dtype.kind == "f":
        return np.isnan(a)
    if a.dtype.kind in "iub":
        return np.zeros(a.shape, dtype=bool)
    return np.array([v is None or v != v for v in a.tolist()], dtype=bool)


def nearest_grid(grid_lat, grid_lon, lat, lon) -> tuple[np.ndarray, np.ndarray]:
    from scipy.spatial import cKDTree

    lon_wrapped = np.where(np.asarray(grid_lon) > 180, np.asarray(grid_lon) - 360, grid_lon)
    return cKDTree(np.column_stack([grid_lat, lon_wrapped])).query(np.column_stack([lat, lon]))


def superob(table: dict, grid_lat, grid_lon, timeslot_length: int, nearest=(), groupby=()) -> dict:
    """The thinned table as a dict ``name -> array`` in the statement's column and row order."""
    table = {k: np.asarray(v) for k, v in table.items()}
    keep = ~(is_missing(table["date"]) | is_missing(table["latitude"]) | is_missing(table["longitude"]))
    table = {k: v[keep] for k, v in table.items()}
    if not keep.any():
        return table
    distance, spatial = nearest_grid(grid_lat, grid_lon, table["latitude"], table["longitude"])
    ns = table["date"].astype("datetime64[ns]").view(np.int64)
    temporal = (ns - ns.min()) // (int(timeslot_length) * 10**9)
    table.update(grid_index=spatial + len(grid_lat) * temporal, spatial_index=spatial.astype(np.int64), distance=distance)
    key_names = ["grid_index", *groupby]
    averaged = [c for c in table if c not in key_names and c not in nearest]
    # groups in order of first appearance
    key_missing = np.zeros(len(ns), dtype=bool)
    for name in key_names:
        key_missing |= is_missing(table[name])
    key_columns = [table[name].tolist() for name in key_names]
    number: dict[tuple, int] = {}
    members: list[list[int]] = []
    for r in range(len(ns)):
        if key_missing[r]:
            continue
        g = number.setdefault(tuple(col[r] for col in key_columns), len(members))
        if g == len(members):
            members.append([])
        members[g].append(r)
    out: dict[str, list] = {name: [] for name in [*groupby, *averaged, *nearest]}
    for rows in members:
        rows = np.array(rows)
        for name in groupby:
            out[name].append(table[name][rows[0]])
        for name in averaged:
            col = table[name][rows]
            if col.dtype.kind == "M":
                v = col.astype("datetime64[ns]").view(np.int64)
                mean, count = kahan_mean(np.where(v == NAT, np.nan, v.astype(np.float64)))
                out[name].append(np.int64(NAT if count == 0 else int(mean)))  # int(): truncation, as the cast to int64
            elif col.dtype.kind in "iubf":
                out[name].append(kahan_mean(col.astype(np.float64))[0])
            else:
                raise TypeError(f"column {name!r} cannot be averaged")
        d = table["distance"][rows]
        best = rows[0]
        best_d = np.inf
        found = False
        for r, v in zip(rows.tolist(), d.tolist()):  # strict <: the first of equals
            if v < best_d or (not found and v == v):
                best, best_d, found = r, v, True
        for name in nearest:
            out[name].append(table[name][best])
    result = {}
    for name, vals in out.items():
        src = table[name]
        if name in averaged:
            result[name] = np.array(vals, dtype=np.int64).view("datetime64[ns]") if src.dtype.kind == "M" else np.array(vals, dtype=np.float64)
        else:
            result[name] = np.array(vals, dtype=src.dtype)
    del result["distance"]
    when = result["date"].astype("datetime64[ns]").view(np.int64)
    by_date = np.argsort(np.where(when == NAT, np.iinfo(np.int64).max, when), kind="stable")
    return {name: v[by_date] for name, v in result.items()}


# ---- seeded tables ---------------------------------------------------------------------------------------------------------------
def random_table(seed: int, n: int | None = None, big_group: int = 0, with_strings: bool = False) -> tuple[dict, dict]:
    """``(table, config)``: a seeded table over the 5-degree lat-lon grid's neighbourhood with what a test of the mean needs: NaN
    and +-inf in value columns, magnitudes over 16 decades, an int64 column, a second datetime column (averaged), a group-by column
    with missing entries, crowded cells, and — ``big_group`` > 0 — that many rows in ONE cell, slot and report type."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(400, 3000)) if n is None else n
    n_sites = max(4, n // int(rng.integers(20, 80)))
    site_lat, site_lon = rng.uniform(-88, 88, n_sites), rng.uniform(-179, 179, n_sites)
    site = rng.integers(0, n_sites, n)
    if big_group:
        site[rng.choice(n, big_group, replace=False)] = 0
    jitter = np.where(site == 0, 0.01, 0.4) if big_group else 0.4  # the big group stays in one cell
    lat = site_lat[site] + rng.uniform(-1, 1, n) * jitter
    lon = site_lon[site] + rng.uniform(-1, 1, n) * jitter
    base = np.datetime64("2025-01-01T00:00:00", "ns")
    seconds = rng.integers(0, 3 * 3600, n)
    if big_group:
        seconds[site == 0] = rng.integers(0, 600, int((site == 0).sum()))  # one time slot
    date = base + seconds * np.timedelta64(10**9, "ns")
    report = rng.choice([1001.0, 1002.0, 16005.0], n)
    report[rng.random(n) < 0.02] = np.nan
    if big_group:
        report[site == 0] = 1001.0
    table = {"date": date, "latitude": lat, "longitude": lon, "reportype": report}
    table["wide"] = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)  # 16 decades
    table["wide"][rng.random(n) < 0.1] = np.nan
    extremes = rng.standard_normal(n) * 250.0
    extremes[rng.random(n) < 0.05] = np.nan
    extremes[rng.choice(n, 3, replace=False)] = [np.inf, -np.inf, np.inf]
    table["extremes"] = extremes
    table["near"] = 1e15 + rng.integers(0, 1000, n) * 0.125 + rng.standard_normal(n) * 1e-3  # cancellation: what the compensation is for
    table["counts"] = rng.integers(-2**40, 2**40, n).astype(np.int64)
    seen = base + rng.integers(0, 10**13, n) * np.timedelta64(1, "ns")
    seen[rng.random(n) < 0.05] = np.datetime64("NaT")
    table["seen"] = seen
    for name, rows in (("date", 2), ("latitude", 2), ("longitude", 1)):
        at = rng.choice(n, rows, replace=False)
        table[name] = table[name].copy()
        table[name][at] = np.datetime64("NaT") if name == "date" else np.nan
    if with_strings:
        table["station"] = rng.choice(np.array(["a", "bb", "ccc"], dtype=object), n)
        if big_group:
            table["station"][site == 0] = "a"
    config = {"grid": "5/5" if seed % 2 else "o32", "timeslot_length": int(rng.choice([900, 3600, 7200])),
              "columns_to_take_nearest": ["date"] if seed % 3 else ["date", "counts"],
              "columns_to_groupby": (["reportype"] if seed % 4 else []) + (["station"] if with_strings else [])}
    return table, config


def canonical(columns: dict) -> dict:
    """Rows ordered by date and then by every other column (NaN / NaT last), for comparing two routes that leave tied dates in
    different orders."""
    names = list(columns)
    keys = []
    for name in reversed(["date"] + [c for c in names if c != "date"]):
        v = np.asarray(columns[name])
        if v.dtype.kind == "M":
            v = v.astype("datetime64[ns]").view(np.int64)
            v = np.where(v == NAT, np.iinfo(np.int64).max, v)
        elif v.dtype.kind == "O":
            v = np.unique(v.astype(str), return_inverse=True)[1]
        elif v.dtype.kind == "f":
            keys.append(np.nan_to_num(v, nan=0.0, posinf=np.finfo(np.float64).max, neginf=-np.finfo(np.float64).max))
            v = np.isnan(v)
        keys.append(v)
    # np.lexsort: the LAST key is the primary one
    order = np.lexsort(keys)
    return {name: np.asarray(columns[name])[order] for name in names}


# ---- the golden file ---------------------------------------------------------------------------------------------------------------
def load_golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


def decode_column(spec: dict) -> np.ndarray:
    """A stored column: ``{"kind": "f8" | "i8" | "M8[ns]", "bits": [...]}`` — int64 bit patterns, so that equality is exact."""
    bits = np.array(spec["bits"], dtype=np.int64)
    if spec["kind"] == "f8":
        return bits.view(np.float64)
    if spec["kind"] == "M8[ns]":
        return bits.view("datetime64[ns]")
    return bits


def encode_column(values) -> dict:
    a = np.asarray(values)
    if a.dtype.kind == "f":
        return {"kind": "f8", "bits": a.astype(np.float64).view(np.int64).tolist()}
    if a.dtype.kind == "M":
        return {"kind": "M8[ns]", "bits": a.astype("datetime64[ns]").view(np.int64).tolist()}
    return {"kind": "i8", "bits": a.astype(np.int64).tolist()}


def golden_table(case: dict) -> dict:
    if "table" in case:
        return {name: decode_column(spec) for name, spec in case["table"].items()}
    return random_table(case["seed"], n=case["rows"], big_group=case.get("big_group", 0))[0]


def golden_expected(case: dict) -> dict:
    return {name: decode_column(spec) for name, spec in case["expected"].items()}
