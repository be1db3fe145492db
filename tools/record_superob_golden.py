#!/usr/bin/env python
"""Record tests/golden/superob.json from the reference's own code.

    python tools/record_superob_golden.py /path/to/anemoi-transform/src

Loads TWO files of the reference, ``anemoi/transform/filters/tabular/superob.py`` and ``.../tabular/support/superob.py``, with
stand-ins for what they import and do not need here (``healpy``, the filter base class and registry) and with ``lookup`` answered
by this package's formula grids, runs the reference's ``SuperOb.forward`` on the two tables of its own tests
(tests/tabular_filters/test_superob.py) and on seeded random tables (``tests/superob_restatement.random_table``), and stores the
tables and the frames it returned.  Every column is stored as int64 bit patterns (float64 and datetime64[ns] reinterpreted), so
that equality is exact.  Needs pandas and scipy.  Run by no test.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

# (id, seed, rows)
SEEDED = [("seeded_o32_no_groupby", 3100, 260), ("seeded_latlon_groupby_two_nearest", 3105, 240)]


def reference_tables() -> list[tuple[str, dict, dict]]:
    """R: tests/tabular_filters/test_superob.py — the two tables, transcribed."""
    config = {"grid": "o96", "timeslot_length": 3600, "columns_to_take_nearest": ["date"], "columns_to_groupby": ["reportype"]}
    date = np.array(["2025-01-01T00:00:00", "2025-01-01T00:00:01", "2025-01-01T02:00:01", "2025-01-01T02:00:02"], dtype="datetime64[ns]")
    one = {"date": date, "latitude": np.array([89.1, 89.3, 89.2, 89.2]), "longitude": np.array([-126.0, -126.0, -90.0, -90.0]),
           "reportype": np.array([1001, 1001, 1001, 1001]), "obsvalue_rawbt_1": np.array([207, 209, 265, 266])}
    two = {"date": date, "latitude": np.array([89.1, 89.3, 89.2, 89.2]), "longitude": np.array([-126.1, -126.3, -90.0, -90.0]),
           "reportype": np.array([1001, 1001, 1001, 1002]), "obsvalue_rawbt_1": np.array([207, 209, 265, 266])}
    return [("reference_test_superob", one, config), ("reference_test_superob_groupby", two, config)]


def load_reference(src: str):
    """The reference's SuperOb class, from its two files alone."""
    import __graft_entry__ as entry

    entry.load_package()
    from anemoi_transform_amd.grids import lookup

    class Registry:
        def register(self, name):
            return lambda cls: cls

    class Filter:
        def __call__(self, data):
            return self.forward(data)

    stand_ins = {
        "healpy": {},
        "anemoi": {},
        "anemoi.transform": {},
        "anemoi.transform.filter": {"Filter": Filter},
        "anemoi.transform.filters": {},
        "anemoi.transform.filters.tabular": {"filter_registry": Registry()},
        "anemoi.transform.filters.tabular.support": {},
        "anemoi.transform.grids": {},
        "anemoi.transform.grids.named": {"lookup": lookup},
    }
    for name, members in stand_ins.items():
        module = types.ModuleType(name)
        module.__path__ = []  # a package, so that dotted imports below it resolve through sys.modules
        module.__dict__.update(members)
        sys.modules[name] = module
    tabular = os.path.join(src, "anemoi", "transform", "filters", "tabular")
    for name, path in (("anemoi.transform.filters.tabular.support.superob", os.path.join(tabular, "support", "superob.py")),
                       ("reference_superob", os.path.join(tabular, "superob.py"))):
        spec = importlib.util.spec_from_file_location(name, path)
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return module.SuperOb


def main() -> None:
    import pandas as pd

    import superob_restatement as R

    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("reference_src", help="the src/ directory of an anemoi-transform checkout")
    parser.add_argument("--out", default=R.GOLDEN)
    args = parser.parse_args()
    SuperOb = load_reference(args.reference_src)
    tables = reference_tables() + [(name, *R.random_table(seed, n=rows)) for name, seed, rows in SEEDED]
    cases = []
    for name, table, config in tables:
        frame = SuperOb(**config)(pd.DataFrame(table).copy())
        cases.append({"id": name, "config": config, "table": {c: R.encode_column(v) for c, v in table.items()},
                      "expected": {c: R.encode_column(frame[c].to_numpy()) for c in frame.columns},
                      "expected_dtypes": {c: str(frame[c].dtype) for c in frame.columns}})
        print(f"{name}: {len(table['date'])} rows -> {len(frame)} rows, columns {list(frame.columns)}")
    with open(args.out, "w") as f:
        # one line per case keeps the file small and diffs readable
        f.write('{\n "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in cases) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
