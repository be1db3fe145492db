#!/usr/bin/env python
"""Record tests/golden/fill_heights.json from the reference's own code.

    python tools/record_fill_heights_golden.py /path/to/anemoi-transform/src

Loads TWO files of the reference — the filter module ``anemoi/transform/filters/tabular/fill_heights.py`` and
``support/utils.py`` with its ``get_heights`` — with stand-ins for the filter base class and the registry (and for the xarray module
where it is not installed), patches ``xr.open_dataset`` of the filter module as the reference's own tests patch it
(tests/tabular_filters/test_fill_heights.py) so that it hands out the case's orography, and stores for every case the orography, the
table, the altitude column of the frame ``FillHeights.forward`` returned and what ``get_heights`` itself returns for the rows to fill.
The cases: the four of the reference's test file, transcribed below with their expected literals; seeded tables
(``tests/fill_heights_restatement.rows``) against ascending, descending and shuffled axes with float32 and float64 heights; and a block
of rows exactly half-way between two axis entries, where the tree's answer is an artefact of its build.  Floating-point arrays are stored
as integer bit patterns, so that equality is exact.  Needs pandas and scipy.  Run by no test, and never where the reference is absent.
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import types
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLDEN_SHAPE = (19, 36)  # a ten-degree grid: small enough to store
GOLDEN_ROWS = 48


def reference_cases() -> list[dict]:
    """The inputs and expected literals of the reference's test file."""
    table = {"latitude": np.array([-45.0, -45.0, 45.0, 45.0]), "longitude": np.array([0.0, 180.0, 0.0, 180.0])}
    stalt = np.array([np.nan, 9999.0, 3.0, np.nan])
    lat_axis, lon_axis, z = np.array([-45.0, 45.0]), np.array([0.0, 180.0]), np.array([[1.0, 2.0], [3.0, 4.0]])
    orography = dict(lat_axis=lat_axis, lon_axis=lon_axis, heights=z)
    path = "/path/to/orography.zarr"
    return [
        dict(id="reference_test_fill_heights_defaults", config={"orography_file": path}, table={**table, "stalt": stalt}, column="stalt",
             literals=[1.0, 2.0, 3.0, 4.0], **orography),
        dict(id="reference_test_fill_heights_station_altitude", config={"orography_file": path, "station_altitude": "my_station_altitude"},
             table={**table, "my_station_altitude": stalt}, column="my_station_altitude", literals=[1.0, 2.0, 3.0, 4.0], **orography),
        dict(id="reference_test_fill_heights_orog_file_varnames",
             config={"orography_file": path, "orography_altitude": "orog", "orography_latitude": "lat", "orography_longitude": "lon"},
             table={**table, "stalt": stalt}, column="stalt", literals=[1.0, 2.0, 3.0, 4.0], **orography),
        dict(id="reference_test_fill_heights_missing_station_altitude", config={"orography_file": path, "station_altitude": "stalt"},
             table=dict(table), column="stalt", raises="ValueError", **orography),
    ]


def seeded_cases() -> list[dict]:
    import fill_heights_restatement as R

    cases = []
    n_lat, n_lon = GOLDEN_SHAPE
    for k, (kind, dtype) in enumerate([(kind, dtype) for kind in R.KINDS for dtype in (np.float32, np.float64)]):
        lat_axis, lon_axis = R.axes(kind, n_lat, n_lon)
        cases.append(dict(id=f"seeded_{kind}_{np.dtype(dtype).name}", config={"orography_file": "orography.zarr"}, column="stalt",
                          table=R.rows(GOLDEN_ROWS, seed=100 + k), lat_axis=lat_axis, lon_axis=lon_axis,
                          heights=R.heights(n_lat, n_lon, dtype, seed=200 + k)))
    lat_axis, lon_axis = R.midpoint_axes()
    cases.append(dict(id="midpoints", config={"orography_file": "orography.zarr"}, column="stalt", table=R.midpoint_rows(),
                      lat_axis=lat_axis, lon_axis=lon_axis, heights=R.heights(lat_axis.size, lon_axis.size, np.float32, seed=300)))
    return cases


def load_reference(src: str):
    """``(FillHeights, get_heights, the filter's module)`` from the reference's own files."""

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
        "anemoi.transform.filters.tabular.support": {},
    }
    if importlib.util.find_spec("xarray") is None:  # the module only has to exist: open_dataset is patched for every case
        stand_ins["xarray"] = {"open_dataset": None}
    for name, members in stand_ins.items():
        module = types.ModuleType(name)
        module.__path__ = []  # a package, so that dotted imports below it resolve through sys.modules
        module.__dict__.update(members)
        sys.modules[name] = module
    tabular = os.path.join(src, "anemoi", "transform", "filters", "tabular")
    base = "anemoi.transform.filters.tabular"
    loaded = {}
    for name, path in ((f"{base}.support.utils", "support/utils.py"), (f"{base}.fill_heights", "fill_heights.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(tabular, path))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
        loaded[name] = module
    return registry.classes["fill_orography"], loaded[f"{base}.support.utils"].get_heights, loaded[f"{base}.fill_heights"]


def main() -> None:
    import pandas as pd

    import fill_heights_restatement as R

    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("reference_src", help="the src/ directory of an anemoi-transform checkout")
    parser.add_argument("--out", default=R.GOLDEN)
    args = parser.parse_args()
    FillHeights, get_heights, module = load_reference(args.reference_src)
    records = []
    for case in reference_cases() + seeded_cases():
        config = case["config"]
        dataset = {config.get("orography_latitude", "latitude"): case["lat_axis"], config.get("orography_longitude", "longitude"): case["lon_axis"],
                   config.get("orography_altitude", "z"): case["heights"]}
        record = {"id": case["id"], "config": config, "column": case["column"], "lat_axis": R.encode(case["lat_axis"]),
                  "lon_axis": R.encode(case["lon_axis"]), "heights": R.encode(case["heights"]),
                  "table": {c: R.encode(v) for c, v in case["table"].items()}}
        with mock.patch.object(module.xr, "open_dataset") as open_dataset:
            open_dataset.return_value = dataset
            try:
                frame = FillHeights(**config)(pd.DataFrame(case["table"]).copy())
            except ValueError:
                assert case.get("raises") == "ValueError", case["id"]
                record.update(raises="ValueError", expected=R.encode(np.zeros(0)), direct=R.encode(np.zeros(0)))
                records.append(record)
                print(f"{case['id']}: ValueError")
                continue
            open_dataset.assert_called_once_with(config["orography_file"])
        assert "raises" not in case and list(frame.columns) == list(case["table"]), case["id"]
        for name, column in case["table"].items():  # the other columns come back as they went in
            assert name == case["column"] or np.array_equal(frame[name].to_numpy(), column), (case["id"], name)
        rows = np.flatnonzero(R.to_fill(case["table"][case["column"]]))
        direct = get_heights(case["lat_axis"], case["lon_axis"], case["heights"], case["table"]["latitude"][rows], case["table"]["longitude"][rows])
        record.update(expected=R.encode(frame[case["column"]].to_numpy()), direct=R.encode(direct))
        if "literals" in case:
            record["literals"] = case["literals"]
            assert np.allclose(frame[case["column"]].to_numpy(), case["literals"]), case["id"]
        records.append(record)
        print(f"{case['id']}: {len(frame)} rows, {rows.size} filled")
    with open(args.out, "w") as f:
        # one line per case keeps the file small and diffs readable
        f.write('{\n "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in records) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
