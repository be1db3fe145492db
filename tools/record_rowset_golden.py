#!/usr/bin/env python
"""Record tests/golden/rowset.json from the reference's own code.

    python tools/record_rowset_golden.py /path/to/anemoi-transform/src

Loads THREE files of the reference — ``anemoi/transform/filters/tabular/sort_by.py``, ``drop_duplicates.py`` and ``drop.py`` — with
stand-ins for the filter base class, the registry and the missing-column check of ``support/utils.py``, runs their own ``forward`` on
every case and stores the table that went in (once per table) and, per case, the index labels of the frame that came out with a
sha256 digest of its columns' bytes (the labels are unique, so the frame is the table's rows at those labels; the digest pins it).
The cases: the value cases of the reference's three test files, transcribed below with their literals, and the seeded tables
of ``tests/rowset_restatement.py`` (48 and 300 rows; float64, float32, int64, bool, datetime and string columns holding every
special) under seven sort configurations and five duplicate configurations each.  float64 and float32 columns are stored as integer
bit patterns, so that equality is exact.  Needs pandas.  Run by no test, and never where the reference is absent.
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]


def reference_cases() -> tuple[dict, list[dict]]:
    """The inputs of the reference's test files (``tables``, by name) and its cases; ``literals`` are the frames its tests state."""
    xyz = {"x": np.array([0, 1, 1, 1, 0, 0]), "y": np.array([0, 1, 1, 0, 0, 1]), "z": np.array([0, 0, 1, 1, 0, 1])}
    tables = {
        "reference_sort_by": {"col1": np.array([2, 1, 2, 3, 3]), "col2": np.array([4, 5, 3, 2, 1]), "col3": np.array([0, 1, 2, 3, 4])},
        "reference_drop_duplicates": xyz,
        "reference_drop_duplicates_prefix": {"x": xyz["x"], "obsvalue_y": xyz["y"], "obsvalue_z": xyz["z"]},
        "reference_drop": {"x": np.array([0, 1, 2]), "drop_me": np.array([3, 4, 5])},
    }
    cases = [
        dict(id="reference_test_sort_by", filter="sort_by", config={"columns": ["col1", "col2"]}, table="reference_sort_by",
             literals={"col1": [1, 2, 2, 3, 3], "col2": [5, 3, 4, 1, 2], "col3": [1, 2, 0, 4, 3]}),
        dict(id="reference_test_drop_duplicates", filter="drop_duplicates", config={"columns": ["y", "z"]}, table="reference_drop_duplicates",
             dropped_index=[4, 5]),
        dict(id="reference_test_drop_duplicates_with_prefix", filter="drop_duplicates", config={"column_prefix": "obsvalue_"},
             table="reference_drop_duplicates_prefix", dropped_index=[4, 5]),
        dict(id="reference_test_drop_duplicates_no_config", filter="drop_duplicates", config={}, table="reference_drop_duplicates",
             dropped_index=[4]),
        dict(id="reference_test_drop", filter="drop", config={"columns": ["drop_me"]}, table="reference_drop"),
    ]
    return tables, cases


def load_reference(src: str) -> dict:
    """The reference's ``SortBy``, ``DropDuplicates`` and ``Drop`` from their own files, by registered name."""

    class Registry:
        def __init__(self):
            self.classes = {}

        def register(self, name):
            def keep(cls):
                self.classes[name] = cls
                return cls

            return keep

    class Filter:
        def __call__(self, data):
            return self.forward(data)

    def raise_if_df_missing_cols(df, required_cols):
        missing = set(required_cols) - set(df.columns)
        if missing:
            raise ValueError(f"DataFrame is missing columns: {missing}")

    registry = Registry()
    stand_ins = {
        "anemoi": {},
        "anemoi.transform": {},
        "anemoi.transform.filter": {"Filter": Filter},
        "anemoi.transform.filters": {},
        "anemoi.transform.filters.tabular": {"filter_registry": registry},
        "anemoi.transform.filters.tabular.support": {},
        "anemoi.transform.filters.tabular.support.utils": {"raise_if_df_missing_cols": raise_if_df_missing_cols},
    }
    for name, members in stand_ins.items():
        module = types.ModuleType(name)
        module.__path__ = []  # a package, so that dotted imports below it resolve through sys.modules
        module.__dict__.update(members)
        sys.modules[name] = module
    for stem in ("sort_by", "drop_duplicates", "drop"):
        name = f"anemoi.transform.filters.tabular.{stem}"
        spec = importlib.util.spec_from_file_location(name, os.path.join(src, "anemoi", "transform", "filters", "tabular", f"{stem}.py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return registry.classes


def main() -> None:
    import pandas as pd

    import rowset_restatement as R

    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("reference_src", help="the src/ directory of an anemoi-transform checkout")
    parser.add_argument("--out", default=R.GOLDEN)
    args = parser.parse_args()
    classes = load_reference(args.reference_src)

    tables, cases = reference_cases()
    frames = {name: pd.DataFrame(columns) for name, columns in tables.items()}
    for n in R.SEEDED_ROWS:
        table = R.seeded_table(n)
        frames[f"seeded_{n}"] = pd.DataFrame({c: v for c, v in table.items() if c != "label"}, index=table["label"])
    for case in R.seeded_cases():
        cases.append(dict(id=case["id"], filter=case["filter"], config=case["config"], table=f"seeded_{case['rows']}", columns=case["columns"]))

    records = []
    for case in cases:
        before = frames[case["table"]]
        before = before[case["columns"]] if "columns" in case else before
        kept = before.copy(deep=True)
        frame = classes[case["filter"]](**case["config"])(before.copy())
        assert before.equals(kept), case["id"]
        if "literals" in case:  # R: tests/tabular_filters/test_sort_by.py:41-49
            assert frame.reset_index(drop=True).equals(pd.DataFrame({c: np.array(v) for c, v in case["literals"].items()})), case["id"]
        if "dropped_index" in case:  # R: tests/tabular_filters/test_drop_duplicates.py:38, :77, :95
            assert frame.equals(before.drop(index=case["dropped_index"])), case["id"]
        record = {"id": case["id"], "filter": case["filter"], "config": case["config"], "table": case["table"],
                  "columns": list(before.columns), "index": [int(i) for i in frame.index],
                  "expected_columns": list(frame.columns), "digest": R.digest({c: frame[c].to_numpy() for c in frame.columns})}
        record.update({key: case[key] for key in ("literals", "dropped_index") if key in case})
        records.append(record)
        print(f"{case['id']}: {len(before)} -> {len(frame)} rows, columns {list(frame.columns)}")
    stored = {name: {"index": [int(i) for i in frame.index], "columns": {c: R.encode(frame[c].to_numpy()) for c in frame.columns}}
              for name, frame in frames.items()}
    with open(args.out, "w") as f:
        # one line per table and case keeps the file small and diffs readable
        f.write('{\n "tables": {\n' + ",\n".join(f"  {json.dumps(n)}: " + json.dumps(t, separators=(",", ":")) for n, t in stored.items()) + "\n },\n")
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in records) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
