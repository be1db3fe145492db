#!/usr/bin/env python
"""Record tests/golden/column_transformations.json from the reference's own code.

    python tools/record_column_transformations_golden.py /path/to/anemoi-transform/src

Loads ONE file of the reference — ``anemoi/transform/filters/tabular/apply_column_transformations.py`` — with stand-ins for the filter
base class and the registry, runs its own ``ApplyColumnTransformations.forward`` on every case and stores the table that went in and the
frame that came out.  The cases: the four value cases of the reference's test file, transcribed below with their literals; a seeded
frame of 48 rows per function (``tests/column_ops_restatement.cases``, specials included), into a new column and in place; a chained
configuration; and an int64 column through ``abs`` and through ``safe_log``.  float64 columns are stored as integer bit patterns, so
that equality is exact.  Needs pandas.  Run by no test, and never where the reference is absent.
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
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]  # the restatement, and the oracle package its exact values import

GOLDEN_ROWS = 48


def reference_cases() -> list[dict]:
    """The inputs of the reference's test file; ``literals`` are the values its tests state, ``numpy`` the function whose value of the
    input column they compare with."""
    ramp = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    names = ["log", "log1p", "sqrt", "exp", "abs", "sin", "cos"]
    angles = {"col1": np.array([0.0, 90.0, 180.0, 270.0, 360.0]), "col2": np.array([0, 1, 2, 3, 4])}
    return [
        dict(id="reference_test_apply_column_transformations", config={f"col{k + 1}": {"function": f} for k, f in enumerate(names)},
             table={f"col{k + 1}": ramp.copy() for k in range(len(names))}, numpy={f"col{k + 1}": f for k, f in enumerate(names)}),
        dict(id="reference_test_add_sine", config={"sin_col1": {"function": "sin_deg", "source_column": "col1"}}, table=dict(angles),
             literals={"sin_col1": [0.0, 1.0, 0.0, -1.0, 0.0]}),
        dict(id="reference_test_add_cosine", config={"cos_col1": {"function": "cos_deg", "source_column": "col1"}}, table=dict(angles),
             literals={"cos_col1": [1.0, 0.0, -1.0, 0.0, 1.0]}),
        dict(id="reference_test_safe_log", config={"log_col1": {"function": "safe_log", "source_column": "col1"}},
             table={"col1": np.array([0, 1, 2, 3, 4])}, numpy={"log_col1": "safe_log"}),
    ]


def seeded_cases() -> list[dict]:
    import column_ops_restatement as R

    out = []
    for function in R.FUNCTIONS:
        x = R.cases(function)
        rng = np.random.default_rng(500 + R.FUNCTIONS.index(function))
        col = np.concatenate([x[rng.choice(x.size, GOLDEN_ROWS - R.SPECIALS.size, replace=False)], R.SPECIALS])
        assert col.size == GOLDEN_ROWS
        out.append(dict(id=f"seeded_{function}", table={"x": col, "other": np.arange(GOLDEN_ROWS)},
                        config={f"{function}_of_x": {"function": function, "source_column": "x"}, "x": {"function": function}}))
    rng = np.random.default_rng(77)
    out.append(dict(id="chained", table={"sp": rng.uniform(5.0e4, 1.05e5, GOLDEN_ROWS), "dd": rng.uniform(0.0, 360.0, GOLDEN_ROWS),
                                         "tp": np.where(rng.random(GOLDEN_ROWS) < 0.3, 0.0, rng.gamma(0.5, 2.0, GOLDEN_ROWS))},
                    config={"lnsp": {"function": "safe_log", "source_column": "sp"}, "sp_again": {"function": "exp", "source_column": "lnsp"},
                            "sin_dd": {"function": "sin_deg", "source_column": "dd"}, "cos_dd": {"function": "cos_deg", "source_column": ["dd"]},
                            "dd": {"function": "sqrt"}, "tp": {"function": "log1p"}, "root": {"function": "sqrt", "source_column": "sin_dd"},
                            "lnsp_abs": {"function": "abs", "source_column": "lnsp"}, "wave": {"function": "cos", "source_column": "dd"}}))
    ints = np.concatenate([rng.integers(-1000, 1000, GOLDEN_ROWS - 4), [0, -1, np.iinfo(np.int64).max, np.iinfo(np.int64).min + 1]]).astype(np.int64)
    out.append(dict(id="int64_abs_and_safe_log", table={"k": ints, "x": rng.normal(0.0, 1.0, GOLDEN_ROWS)},
                    config={"k_abs": {"function": "abs", "source_column": "k"}, "k_log": {"function": "safe_log", "source_column": "k_abs"},
                            "k": {"function": "abs"}, "k_sin": {"function": "sin", "source_column": "k"}}))
    return out


def load_reference(src: str):
    """The reference's ``ApplyColumnTransformations`` from its own file."""

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

    registry = Registry()
    stand_ins = {
        "anemoi": {},
        "anemoi.transform": {},
        "anemoi.transform.filter": {"Filter": Filter},
        "anemoi.transform.filters": {},
        "anemoi.transform.filters.tabular": {"filter_registry": registry},
    }
    for name, members in stand_ins.items():
        module = types.ModuleType(name)
        module.__path__ = []  # a package, so that dotted imports below it resolve through sys.modules
        module.__dict__.update(members)
        sys.modules[name] = module
    name = "anemoi.transform.filters.tabular.apply_column_transformations"
    path = os.path.join(src, "anemoi", "transform", "filters", "tabular", "apply_column_transformations.py")
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return registry.classes["apply_column_transformations"]


def main() -> None:
    import pandas as pd

    import column_ops_restatement as R

    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("reference_src", help="the src/ directory of an anemoi-transform checkout")
    parser.add_argument("--out", default=R.GOLDEN)
    args = parser.parse_args()
    ApplyColumnTransformations = load_reference(args.reference_src)
    records = []
    for case in reference_cases() + seeded_cases():
        before = pd.DataFrame(case["table"])
        with np.errstate(all="ignore"):
            frame = ApplyColumnTransformations(**case["config"])(before.copy())
        assert before.equals(pd.DataFrame(case["table"])), case["id"]
        record = {"id": case["id"], "config": case["config"], "table": {c: R.encode(v) for c, v in case["table"].items()},
                  "expected": {c: R.encode(frame[c].to_numpy()) for c in frame.columns}}
        for column, values in case.get("literals", {}).items():
            assert np.allclose(frame[column].to_numpy(), values), (case["id"], column)
        for column, function in case.get("numpy", {}).items():
            source = case["config"][column].get("source_column", column)
            with np.errstate(all="ignore"):
                assert np.allclose(frame[column].to_numpy(), R.NUMPY[function](case["table"][source]), equal_nan=True), (case["id"], column)
        record.update({key: case[key] for key in ("literals", "numpy") if key in case})
        records.append(record)
        print(f"{case['id']}: {len(frame)} rows, columns {list(frame.columns)}")
    with open(args.out, "w") as f:
        # one line per case keeps the file small and diffs readable
        f.write('{\n "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in records) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
