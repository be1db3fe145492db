#!/usr/bin/env python
"""Record the ``random_cases`` of tests/golden/irregular_to_grid.json from the reference's own code.

    python tools/record_irregular_to_grid_golden.py /path/to/anemoi-transform/src

Loads ONE file of the reference, ``anemoi/transform/filters/tabular/irregular_to_grid.py``, with stand-ins for the modules it
imports that are not needed for the three functions used here (``earthkit.data``, ``anemoi.utils.window``, the filter base class
and registry), builds seeded random tables with many ties, and stores for each the grids that the reference's ``select_window`` /
``get_nearest_obs`` / ``_fill_grids`` produce, driven target by target as its ``forward`` drives them.  Needs pandas.  Run by no
test; the other keys of the golden file (the transcribed cases of the reference's tests) are kept as they are.

The tables are stored compactly (see ``tests/obs_gridding_restatement.random_case_table``): per row the date and the window date in
steps of whole minutes after ``base``, the cell and a bit mask of NaN columns; the value of column j in row r is r * n_cols + j.
"""

from __future__ import annotations

import argparse
import datetime
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

BASE = "2023-01-01T00:00:00"

# (id, seed, rows, cells, targets every .. minutes, number of targets, date lattice in minutes, window, weight, columns)
CASES = [
    ("ties_default_window_w0", 11, 2000, 64, 360, 8, 30, None, 0.0, ["a", "b", "c"]),
    ("overlapping_window_w03", 12, 2000, 64, 360, 8, 30, "(-9h, +3h]", 0.3, ["a", "b", "c"]),
    ("closed_open_window_w1", 13, 2000, 61, 180, 10, 15, "[-6h, +6h)", 1.0, ["a", "b"]),
]


def load_reference(src: str):
    """The reference's IrregularToGrid class, from its file alone."""
    import __graft_entry__ as entry

    entry.load_package()
    from anemoi_transform_amd import obs

    class Window:
        def __init__(self, text: str) -> None:
            w = obs.parse_window(text)
            self.before = datetime.timedelta(microseconds=w.before_ns // 1000)
            self.after = datetime.timedelta(microseconds=w.after_ns // 1000)
            self.closed = (w.closed_before, w.closed_after)

    class Registry:
        def register(self, name):
            return lambda cls: cls

    def raise_if_df_missing_cols(df, required_cols):
        missing = set(required_cols) - set(df.columns)
        if missing:
            raise ValueError(f"missing columns {missing}")

    stand_ins = {
        "earthkit": {},
        "earthkit.data": {"FieldList": object},
        "anemoi": {},
        "anemoi.utils": {},
        "anemoi.utils.window": {"Window": Window},
        "anemoi.transform": {},
        "anemoi.transform.filter": {"Filter": object},
        "anemoi.transform.filters": {},
        "anemoi.transform.filters.tabular": {"filter_registry": Registry()},
        "anemoi.transform.filters.tabular.support": {},
        "anemoi.transform.filters.tabular.support.utils": {"raise_if_df_missing_cols": raise_if_df_missing_cols},
    }
    for name, members in stand_ins.items():
        module = types.ModuleType(name)
        module.__path__ = []  # a package, so that dotted imports below it resolve through sys.modules
        module.__dict__.update(members)
        sys.modules[name] = module
    path = os.path.join(src, "anemoi", "transform", "filters", "tabular", "irregular_to_grid.py")
    spec = importlib.util.spec_from_file_location("reference_irregular_to_grid", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.IrregularToGrid, Window


def make_case(spec) -> dict:
    name, seed, n, n_cells, spacing, n_targets, lattice, window, weight, columns = spec
    rng = np.random.default_rng(seed)
    span = spacing * (n_targets + 1)
    date_step = rng.integers(0, span // lattice, n)
    window_step = rng.integers(1, n_targets + 1, n)  # the row's own window date: NOT what selects it
    cell = rng.integers(0, n_cells, n)
    cell[rng.integers(0, n, 12)] = rng.choice([-1, n_cells, n_cells + 6, -7], 12)
    # crowd a few cells so that equal scores are common
    crowded = rng.integers(0, n, n // 4)
    cell[crowded] = rng.integers(0, 3, len(crowded))
    nan_mask = np.where(rng.random(n) < 0.35, rng.integers(0, 2 ** len(columns), n), 0)
    nat_rows = sorted(int(r) for r in rng.choice(n, 5, replace=False))
    config = {"window_date_column": "window_date", "time_freq": "6h", "columns": columns, "nan_score_weight": weight}
    if window is not None:
        config["window"] = window
    return {"id": name, "seed": seed, "n_cells": n_cells, "config": config, "base": BASE, "date_step_min": lattice,
            "date_step": date_step.tolist(), "window_step_min": spacing, "window_step": window_step.tolist(), "cell": cell.tolist(), "nan_mask": nan_mask.tolist(), "nat_rows": nat_rows}


def record(case: dict, reference, Window) -> None:
    import pandas as pd

    from obs_gridding_restatement import random_case_table

    config = case["config"]
    columns = config["columns"]
    df = pd.DataFrame(random_case_table(case))
    window = Window(config.get("window") or f"(-{config['time_freq']}, 0]")
    targets = pd.to_datetime(df["window_date"].unique())
    grids = {c: np.full((len(targets), case["n_cells"]), np.nan) for c in columns}
    for t, target in enumerate(targets):
        target = pd.Timestamp(target).tz_localize(None)
        selected = reference.select_window(df, target, columns, window)
        if selected is None:
            continue
        nearest = reference.get_nearest_obs(selected, target, pd.Timedelta(config["time_freq"]), columns, config["nan_score_weight"])
        reference._fill_grids(grids, nearest, columns, case["n_cells"], t)
    # every value is a whole number (a row code): stored as int, NaN as null
    case["expected"] = {c: [[None if np.isnan(v) else int(v) for v in row] for row in grids[c]] for c in columns}


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("reference_src", help="the src/ directory of an anemoi-transform checkout")
    parser.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "irregular_to_grid.json"))
    args = parser.parse_args()
    reference, Window = load_reference(args.reference_src)
    with open(args.out) as f:
        golden = json.load(f)
    golden["random_cases"] = []
    for spec in CASES:
        case = make_case(spec)
        record(case, reference, Window)
        golden["random_cases"].append(case)
        filled = sum(v is not None for rows in case["expected"].values() for row in rows for v in row)
        print(f"{case['id']}: {len(case['date_step'])} rows, {filled} grid values filled")
    with open(args.out, "w") as f:
        # one line per top-level list keeps the file small and diffs readable
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in golden.items()) + "\n}\n")


if __name__ == "__main__":
    main()
