#!/usr/bin/env python
"""Record tests/golden/statids.json from the reference's own code.

    python tools/record_statids_golden.py /path/to/anemoi-transform/src

Loads TWO files of the reference's ``anemoi/transform/filters/tabular/`` — ``encode_statids.py`` and ``rename.py`` — with stand-ins for
the filter base class, the registry and the missing-column check of ``support/utils.py``, and runs their own ``forward`` on a copy of
every table.  Stored: the identifiers that went in, as lists of code points (JSON strings cannot carry a NUL or a lone control byte
readably), and the column that came out with its dtype — values as JSON integers, which hold 2^63 and beyond.  The tables are those
of ``tests/statids_restatement.py``: the edge table, the seeded tables of 48 and 300 rows, and a three-row table with one value of
2^63, which shows pandas' dtype for it.  For every table the kernel's rules (``kernel_rules``: pure numpy) predict the rows the
kernel leaves undecided; the count is stored, and the seeded tables must leave at least 90 % of their rows to the kernel.  The
tabular ``rename`` is run on one small frame.  Needs pandas.  Run by no test, and never where the reference is absent.
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
STEMS = ("encode_statids", "rename")


def load_reference(src: str) -> dict:
    """The reference's two filter classes from their own files, by registered name."""

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

    import statids_restatement as R

    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("reference_src", help="the src/ directory of an anemoi-transform checkout")
    parser.add_argument("--out", default=R.GOLDEN)
    args = parser.parse_args()
    classes = load_reference(args.reference_src)

    tables = {"edge": R.edge_strings(), "overflow": ["1001", "1Y2P0IJ32E8E8", "a-b"]}
    tables.update({f"seeded_{n}": R.seeded_strings(n) for n in R.SEEDED_ROWS})
    # R: tests/tabular_filters/test_encode_statids.py — the three literals the reference's own test states
    literals = {"here": 812282, "there": 49521146, "1001": 46657}
    stored = {}
    for name, strings in tables.items():
        before = pd.DataFrame({"statid": pd.Series(strings, dtype=object), "x": np.arange(len(strings), dtype=np.float64)})
        frame = classes["encode_statids"](station_id="statid")(before.copy(deep=True))
        assert list(frame.columns) == ["statid", "x"] and len(frame) == len(strings), name
        values = [int(v) for v in frame["statid"].tolist()]
        for s, v in zip(strings, values):
            assert s not in literals or v == literals[s], (s, v)
        text, width = R.pack(strings)
        undecided = R.kernel_rules(text, width)[0] if width <= R.MAX_WIDTH else np.ones(len(strings), dtype=bool)
        if name.startswith("seeded_"):
            assert undecided.sum() * 10 <= len(strings), (name, int(undecided.sum()))  # the kernel alone decides at least 90 %
            assert str(frame["statid"].dtype) == "int64", frame["statid"].dtype
        stored[name] = {"strings": R.points_of(strings), "codes": values, "dtype": str(frame["statid"].dtype), "width": width,
                        "undecided": int(undecided.sum())}
        print(f"{name}: {len(strings)} rows, width {width}, dtype {frame['statid'].dtype}, {int(undecided.sum())} undecided by the kernel's rules")

    before = pd.DataFrame({"a": [1.5, 2.5, 3.5], "statid": ["x", "y", "z"], "b": [1, 2, 3]})
    frame = classes["rename_tabular"](columns={"a": "alpha", "b": "a"})(before.copy(deep=True))
    rename = {"columns": {"a": "alpha", "b": "a"}, "before": {c: before[c].tolist() for c in before.columns},
              "after_names": list(frame.columns), "after": [frame.iloc[:, j].tolist() for j in range(frame.shape[1])]}
    with open(args.out, "w") as f:
        f.write('{\n "tables": {\n' + ",\n".join(f"  {json.dumps(n)}: " + json.dumps(t, separators=(",", ":")) for n, t in stored.items()) + "\n },\n")
        f.write(' "rename": ' + json.dumps(rename, separators=(",", ":")) + "\n}\n")


if __name__ == "__main__":
    main()
