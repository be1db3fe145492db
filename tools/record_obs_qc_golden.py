#!/usr/bin/env python
"""Record tests/golden/obs_qc.json from the reference's own code.

    python tools/record_obs_qc_golden.py /path/to/anemoi-transform/src

Loads NINE files of the reference's ``anemoi/transform/filters/tabular/`` — ``mask.py``, ``mask_outside_range.py``, ``mask_infs.py``,
``mask_dewpoint_temperature.py``, ``exclude_dates.py``, ``remove_extreme_values.py``, ``clip.py``, ``impute_nans.py`` and ``drop_nans.py`` —
with stand-ins for the filter base class, the registry and the missing-column check of ``support/utils.py``, runs their own ``forward``
on a copy of every case's table and stores the tables that went in (once each; a seeded table as its row count and digest) and, per
case, what came out: the rows that left, the columns that differ from the table's remaining rows (per new value, float64 / float32 as
bit patterns, the rows that hold it), the dtypes that changed and a sha256 digest of the whole frame.  The cases: the value cases of the reference's nine test files, transcribed below with their literals, and
the seeded tables of ``tests/row_program_restatement.py`` (48 and 300 rows) under its configurations.  Needs pandas.  Run by no test,
and never where the reference is absent.
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]
STEMS = ("mask", "mask_outside_range", "mask_infs", "mask_dewpoint_temperature", "exclude_dates", "remove_extreme_values", "clip",
         "impute_nans", "drop_nans")
NAN, INF = float("nan"), float("inf")


def reference_cases() -> tuple[dict, list[dict]]:
    """The inputs of the reference's test files (``tables``, by name) and its value cases; ``literals`` are the columns its tests
    state, ``dropped_index`` the labels they say leave."""
    dates = np.array(["2025-01-01T00:00", "2025-01-02T00:00", "2025-01-02T06:00", "2025-01-03T00:00", "2025-05-04T00:00"], dtype="datetime64[ns]")
    dew = {"2d": np.array([1.0, 2.0, 3.1, NAN, 5.0]), "2t": np.array([1.0, 2.1, 3.0, 4.0, NAN]), "x": np.array([1, 2, 3, 4, 5])}
    extreme = {"latitude": np.array([0.0, 1e4, 1e5, 1e6]), "longitude": np.array([0.0, 1.0, 1e6, 1.0]), "obsvalue_x": np.array([2.0, 1e6, 1.0, 0.0]),
               "fg_deparx": np.array([2.0, 1e6, 1.0, 0.0]), "biascorr_fgx": np.array([2.0, 1e6, 1.0, 0.0]), "pressurex": np.array([2.0, 1e6, 1.0, 0.0]),
               "y": np.array([0.0, 1.0, 2.0, 3.0])}
    nans = {"obsvalue_x": np.array([0.0, NAN, 2.0, NAN, 4.0]), "obsvalue_y": np.array([0.0, 1.0, NAN, NAN, 4.0]), "z": np.array([0.0, 1.0, 2.0, 3.0, NAN])}
    tables = {
        "reference_two_columns": {"col1": np.array([0, 1, 2, 3]), "col2": np.array([3, 4, 5, 6])},
        "reference_infs": {"col1": np.array([INF, 1, 2, -INF]), "col2": np.array([3, INF, -INF, 6])},
        "reference_dewpoint": dew,
        "reference_dewpoint_named": {"obsvalue_td2m_0": dew["2d"], "obsvalue_t2m_0": dew["2t"], "x": dew["x"]},
        "reference_dewpoint_humidity": {"my_td": dew["2d"], "my_t": dew["2t"], "my_q": dew["x"]},
        "reference_dates": {"date": dates, "col1": np.array([0, 1, 2, 3, 4]), "col2": np.array([0, 1, 2, 3, 4])},
        "reference_extreme": {c: extreme[c] for c in ("latitude", "longitude", "obsvalue_x", "y")},
        "reference_extreme_wide": extreme,
        "reference_nans": nans,
        "reference_impute": {"obsvalue_x": np.array([0.0, NAN, 2.0, NAN]), "obsvalue_y": np.array([0.0, 1.0, NAN, NAN]), "z": np.array([0.0, 1.0, 2.0, NAN])},
        "reference_impute_dict": {"obsvalue_x": np.array([0.0, NAN, 2.0]), "obsvalue_y": np.array([0.0, 1.0, NAN])},
        "reference_impute_prefix": {"obsvalue_x": np.array([0.0, NAN, 2.0]), "obsvalue_y": np.array([NAN, 1.0, NAN]), "z": np.array([0.0, 1.0, NAN])},
    }
    two, td = "reference_two_columns", [1.0, 2.0, NAN, NAN, 5.0]
    wide = {"latitude": [0.0, 1e4, 1e5, NAN], "longitude": [0.0, 1.0, NAN, 1.0], "obsvalue_x": [2.0, NAN, 1.0, 0.0]}
    cases = [
        dict(id="reference_test_mask", filter="mask_tabular", config={"col1": {"value": 2, "operator": ">="}}, table=two, literals={"col1": [0, 1, NAN, NAN]}),
        dict(id="reference_test_mask_outside_range", filter="mask_outside_range", config={"col1": [1, 2]}, table=two, literals={"col1": [NAN, 1, 2, NAN]}),
        dict(id="reference_test_mask_outside_range_no_lower_bound", filter="mask_outside_range", config={"col1": [None, 2]}, table=two,
             literals={"col1": [0, 1, 2, NAN]}),
        dict(id="reference_test_mask_outside_range_no_upper_bound", filter="mask_outside_range", config={"col1": [1, None]}, table=two,
             literals={"col1": [NAN, 1, 2, 3]}),
        dict(id="reference_test_mask_infs_with_prefix", filter="mask_infs", config={"column_prefix": "col"}, table="reference_infs",
             literals={"col1": [NAN, 1, 2, NAN], "col2": [3, NAN, NAN, 6]}),
        dict(id="reference_test_mask_infs_with_columns", filter="mask_infs", config={"columns": ["col1"]}, table="reference_infs",
             literals={"col1": [NAN, 1.0, 2.0, NAN]}),
        dict(id="reference_test_mask_dewpoint_temperature_only", filter="mask_dewpoint_temperature", config={"mask_specific_humidity": False},
             table="reference_dewpoint", literals={"2d": td}),
        dict(id="reference_test_mask_dewpoint_temperature_only_column_names", filter="mask_dewpoint_temperature",
             config={"temperature": "obsvalue_t2m_0", "dewpoint_temperature": "obsvalue_td2m_0", "mask_specific_humidity": False},
             table="reference_dewpoint_named", literals={"obsvalue_td2m_0": td}),
        dict(id="reference_test_mask_dewpoint_temperature_with_specific_humidity", filter="mask_dewpoint_temperature",
             config={"temperature": "my_t", "dewpoint_temperature": "my_td", "specific_humidity": "my_q", "mask_specific_humidity": True},
             table="reference_dewpoint_humidity", literals={"my_td": td, "my_q": [1, 2, NAN, 4, 5]}),
        dict(id="reference_test_exclude_dates", filter="exclude_dates", config={"col1": [[20250101, 20250102], [20250105, 20250105]]},
             table="reference_dates", literals={"col1": [NAN, NAN, NAN, 3, 4]}),
        dict(id="reference_test_exclude_dates_single_range", filter="exclude_dates", config={"col1": [20250101, 20250101]}, table="reference_dates",
             literals={"col1": [NAN, 1, 2, 3, 4]}),
        dict(id="reference_test_remove_extreme_values_drop_with_prefix", filter="remove_extreme_values",
             config={"method": "drop", "threshold": 1e5, "column_prefix": "obsvalue_"}, table="reference_extreme", dropped_index=[1, 2, 3]),
        dict(id="reference_test_remove_extreme_values_drop_with_columns", filter="remove_extreme_values",
             config={"method": "drop", "threshold": 1e5, "columns": ["obsvalue_x"]}, table="reference_extreme", dropped_index=[1, 2, 3]),
        dict(id="reference_test_remove_extreme_values_mask_with_prefix", filter="remove_extreme_values",
             config={"method": "mask", "threshold": 1e5, "column_prefix": "obsvalue_"}, table="reference_extreme_wide", literals=wide),
        dict(id="reference_test_remove_extreme_values_mask_with_columns", filter="remove_extreme_values",
             config={"method": "mask", "threshold": 1e5, "columns": ["obsvalue_x", "fg_deparx", "biascorr_fgx", "pressurex"]},
             table="reference_extreme_wide", literals={**wide, "fg_deparx": [2.0, NAN, 1.0, 0.0], "biascorr_fgx": [2.0, NAN, 1.0, 0.0],
                                                       "pressurex": [2.0, NAN, 1.0, 0.0]}),
        dict(id="reference_test_clip", filter="clip_tabular", config={"col1": [1, 2]}, table=two, literals={"col1": [1, 1, 2, 2]}),
        dict(id="reference_test_clip_no_upper", filter="clip_tabular", config={"col1": [1, None]}, table=two, literals={"col1": [1, 1, 2, 3]}),
        dict(id="reference_test_clip_no_lower", filter="clip_tabular", config={"col1": [None, 2]}, table=two, literals={"col1": [0, 1, 2, 2]}),
        dict(id="reference_test_impute_nans_scalar_all_columns", filter="impute_nans_tabular", config={"value": 0.0}, table="reference_impute",
             literals={"obsvalue_x": [0.0, 0.0, 2.0, 0.0], "obsvalue_y": [0.0, 1.0, 0.0, 0.0], "z": [0.0, 1.0, 2.0, 0.0]}),
        dict(id="reference_test_impute_nans_dict_value", filter="impute_nans_tabular", config={"value": {"obsvalue_x": -1.0, "obsvalue_y": -2.0}},
             table="reference_impute_dict", literals={"obsvalue_x": [0.0, -1.0, 2.0], "obsvalue_y": [0.0, 1.0, -2.0]}),
        dict(id="reference_test_impute_nans_with_column_prefix", filter="impute_nans_tabular", config={"value": 99.0, "column_prefix": "obsvalue_"},
             table="reference_impute_prefix", literals={"obsvalue_x": [0.0, 99.0, 2.0], "obsvalue_y": [99.0, 1.0, 99.0]}),
        dict(id="reference_test_drop_nans_all_with_prefix", filter="drop_nans_tabular", config={"column_prefix": "obsvalue_", "how": "all"},
             table="reference_nans", dropped_index=[3]),
        dict(id="reference_test_drop_nans_all_with_columns", filter="drop_nans_tabular", config={"columns": ["obsvalue_x", "obsvalue_y"], "how": "all"},
             table="reference_nans", dropped_index=[3]),
        dict(id="reference_test_drop_nans_any_with_columns", filter="drop_nans_tabular", config={"columns": ["obsvalue_x", "obsvalue_y", "z"], "how": "any"},
             table="reference_nans", dropped_index=[1, 2, 3, 4]),
        dict(id="reference_test_drop_nans_any_with_prefix", filter="drop_nans_tabular", config={"column_prefix": "obsvalue_", "how": "any"},
             table="reference_nans", dropped_index=[1, 2, 3]),
        dict(id="reference_test_drop_any_nans", filter="drop_nans_tabular", config={}, table="reference_nans", dropped_index=[1, 2, 3, 4]),
    ]
    return tables, cases


def load_reference(src: str) -> dict:
    """The reference's nine filter classes from their own files, by registered name."""

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
    for stem in STEMS:
        name = f"anemoi.transform.filters.tabular.{stem}"
        spec = importlib.util.spec_from_file_location(name, os.path.join(src, "anemoi", "transform", "filters", "tabular", f"{stem}.py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return registry.classes


def main() -> None:
    import pandas as pd

    import row_program_restatement as R

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
    cases += R.seeded_cases()

    records = []
    for case in cases:
        before = frames[case["table"]]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # pandas announces the upcasts of integer columns that the filters rely on
            frame = classes[case["filter"]](**case["config"])(before.copy(deep=True))
        assert list(frame.columns) == list(before.columns), case["id"]
        rows = before.loc[frame.index]
        for c, literal in case.get("literals", {}).items():  # R: tests/tabular_filters/test_<filter>.py, the stated columns
            assert np.array_equal(frame[c].to_numpy().astype(np.float64), np.array(literal, dtype=np.float64), equal_nan=True), (case["id"], c)
        if "dropped_index" in case:
            assert frame.equals(before.drop(index=case["dropped_index"])), case["id"]
        kept = before.index.isin(frame.index)
        assert before.index.is_unique and list(before.index[kept]) == list(frame.index), case["id"]  # the survivors, in the table's order
        changed = {c: R.pack_changed(rows[c].to_numpy(), frame[c].to_numpy()) for c in frame.columns
                   if not R.same_bits(frame[c].to_numpy(), rows[c].to_numpy())}
        record = {"id": case["id"], "filter": case["filter"], "config": case["config"], "table": case["table"], "changed": changed,
                  "dtypes": {c: str(frame[c].to_numpy().dtype) for c in frame.columns if frame[c].to_numpy().dtype != before[c].to_numpy().dtype},
                  "digest": R.frame_digest({c: frame[c].to_numpy() for c in frame.columns})}
        if not kept.all():
            record["dropped"] = R.pack_rows(~kept)
        record.update({key: case[key] for key in ("literals", "dropped_index") if key in case})
        records.append(record)
        print(f"{case['id']}: {len(before)} -> {len(frame)} rows, changed {list(changed)}")
    stored = {name: {"index": [int(i) for i in frame.index], "columns": {c: R.encode(frame[c].to_numpy()) for c in frame.columns}}
              for name, frame in frames.items() if not name.startswith("seeded_")}
    stored.update({f"seeded_{n}": {"seeded": n, "digest": R.frame_digest(R.seeded_table(n))} for n in R.SEEDED_ROWS})
    with open(args.out, "w") as f:
        # one line per table and case keeps the file small and diffs readable; NaN literals are written as JSON's NaN
        f.write('{\n "tables": {\n' + ",\n".join(f"  {json.dumps(n)}: " + json.dumps(t, separators=(",", ":")) for n, t in stored.items()) + "\n },\n")
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in records) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
