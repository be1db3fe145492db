#!/usr/bin/env python
"""Record tests/golden/obs_query.json from the reference's own code.

    python tools/record_obs_query_golden.py /path/to/anemoi-transform/src

Loads TWO files of the reference's ``anemoi/transform/filters/tabular/`` — ``filter_query.py`` and ``mask_values_custom.py`` — with the
stand-ins of ``tools/record_obs_qc_golden.py`` for the filter base class, the registry and the missing-column check, runs their own
``forward`` on a copy of every case's table and stores, per table, a digest (the tables themselves are made by
``tests/row_expr_restatement.py``) and, per case, what came out: the rows that left, the columns that differ from the table's remaining
rows (per new value, as bit patterns, the rows that hold it), the dtypes that changed and a sha256 digest of the whole frame.  The
cases (``row_expr_restatement.cases``): the value cases of the reference's two test files, transcribed with their literals; the three
queries of ``filter_query``'s docstring and the one of ``mask_values_custom``'s on a seeded 300-row table; a seeded 48-row table of
int16, int64, uint8, float32, float64, bool and string columns under its queries and masks.  Needs pandas.  Run by no test, and never
where the reference is absent.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
STEMS = ("filter_query", "mask_values_custom")


def main() -> None:
    import record_obs_qc_golden as qc
    import row_expr_restatement as X
    import row_program_restatement as R

    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("reference_src", help="the src/ directory of an anemoi-transform checkout")
    parser.add_argument("--out", default=X.GOLDEN)
    args = parser.parse_args()
    qc.STEMS = STEMS
    classes = qc.load_reference(args.reference_src)

    tables = X.all_tables()
    frames = {name: X.frame_of(t) for name, t in tables.items()}
    records = []
    for case in X.cases():
        before = frames[case["table"]]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # pandas announces the upcasts of integer columns that the filters rely on
            frame = classes[case["filter"]](**case["config"])(before.copy(deep=True))
        assert list(frame.columns) == list(before.columns), case["id"]
        rows = before.loc[frame.index]
        for c, literal in case.get("literals", {}).items():  # R: tests/tabular_filters/test_mask_values_custom.py, the stated column
            assert np.array_equal(frame[c].to_numpy().astype(np.float64), np.array(literal, dtype=np.float64), equal_nan=True), (case["id"], c)
        if "kept_index" in case:  # R: tests/tabular_filters/test_filter_query.py: result.equals(df.iloc[[0, 1]])
            assert frame.equals(before.iloc[case["kept_index"]]), case["id"]
        kept = before.index.isin(frame.index)
        assert before.index.is_unique and list(before.index[kept]) == list(frame.index), case["id"]  # the survivors, in the table's order
        changed = {c: R.pack_changed(rows[c].to_numpy(), frame[c].to_numpy()) for c in frame.columns
                   if not R.same_bits(frame[c].to_numpy(), rows[c].to_numpy())}
        record = {"id": case["id"], "filter": case["filter"], "config": case["config"], "table": case["table"], "changed": changed,
                  "dtypes": {c: str(frame[c].to_numpy().dtype) for c in frame.columns if frame[c].to_numpy().dtype != before[c].to_numpy().dtype},
                  "digest": R.frame_digest({c: frame[c].to_numpy() for c in frame.columns})}
        if not kept.all():
            record["dropped"] = R.pack_rows(~kept)
        record.update({key: case[key] for key in ("literals", "kept_index") if key in case})
        records.append(record)
        print(f"{case['id']}: {len(before)} -> {len(frame)} rows, changed {list(changed)}")
    stored = {name: {"rows": len(t["index"]), "digest": R.frame_digest(t["columns"])} for name, t in tables.items()}
    with open(args.out, "w") as f:
        # one line per table and case keeps the file small and diffs readable; NaN literals are written as JSON's NaN
        f.write('{\n "tables": {\n' + ",\n".join(f"  {json.dumps(n)}: " + json.dumps(t, separators=(",", ":")) for n, t in stored.items()) + "\n },\n")
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in records) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
