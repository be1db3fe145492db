#!/usr/bin/env python
"""Record tests/golden/obs_rowops.json from the reference's own code.

    python tools/record_rowops_golden.py /path/to/anemoi-transform/src

Loads SIX files of the reference — the filter modules ``add_forcings.py``, ``add_azimuth.py``, ``add_msg_angles.py``,
``radiance_to_brightness_temperature.py`` of ``anemoi/transform/filters/tabular/`` and their support modules
``support/compute_forcings.py``, ``support/sat_view_angles.py`` (plus the four lines of ``support/utils.py`` they import) — with
stand-ins for the filter base class and the registry only, runs each filter on the tables of the reference's own tests
(tests/tabular_filters/test_add_forcings.py, test_add_azimuth.py, test_add_msg_angles.py, test_radiance_to_brightness_temperature.py,
transcribed below with their expected literals) and on the seeded tables of ``tests/obs_rowops_restatement.seeded_cases``, and stores
the tables and, of the frames it returned, the column order and every column that is not the table's own.  Every column is stored as int64 bit patterns (float64 and datetime64[ns] reinterpreted), so
that equality is exact.  Needs pandas.  Run by no test.
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


def reference_cases() -> list[dict]:
    """The inputs and expected literals of the reference's four test files."""
    hours = np.array(["2025-01-01T00", "2025-01-01T01", "2025-01-01T02"], dtype="datetime64[ns]")  # pd.date_range("2025-01-01", periods=3, freq="1H")
    points = {"latitude": np.array([-10.0, 0.0, 10.0]), "longitude": np.array([0.0, 90.0, 270.0])}
    spacecraft = {"lat": np.array([-11.0, 1.0, 11.0]), "lon": np.array([1.0, 91.0, 271.0])}
    azimuth = [135.57378316, 44.99563646, 44.42621684]
    msg_azimuth, msg_zenith = [78.703325, 0.0, 90.0], [48.49626885, 51.82994258, 98.60173361]
    sat = np.array([55, 56, 57], dtype=np.int64)
    forcing_columns = ["cos_julian_day", "sin_julian_day", "cos_local_time", "sin_local_time", "cos_sza", "cos_latitude", "sin_latitude",
                       "cos_longitude", "sin_longitude"]
    cases = [
        dict(id="reference_test_add_forcings", filter="add_forcings", config={"columns": forcing_columns},
             table={"date": np.array(["2025-01-01T00:00", "2025-04-01T06:00"], dtype="datetime64[ns]"), "latitude": np.array([-90.0, 90.0]),
                    "longitude": np.array([0.0, 180.0])},
             literals={"cos_julian_day": [1.0, 0.018277], "sin_julian_day": [0.0, 1.0], "cos_local_time": [1.0, 0.0],
                       "sin_local_time": [0.0, -1.0], "cos_sza": [0.391673, 0.075240], "cos_latitude": [0.0, 0.0],
                       "sin_latitude": [-1.0, 1.0], "cos_longitude": [1.0, -1.0], "sin_longitude": [0.0, 0.0]}, rtol=1e-3),
        dict(id="reference_test_add_azimuth", filter="add_azimuth", config={},
             table={**points, "spacecraft_latitude": spacecraft["lat"], "spacecraft_longitude": spacecraft["lon"]}, literals={"azimuth": azimuth}),
        dict(id="reference_test_add_azimuth_with_config", filter="add_azimuth",
             config={"azimuth": "az", "spacecraft_latitude": "sc_lat", "spacecraft_longitude": "sc_lon"},
             table={**points, "sc_lat": spacecraft["lat"], "sc_lon": spacecraft["lon"]}, literals={"az": azimuth}),
        dict(id="reference_test_add_msg_angles_azimuth_default_config", filter="add_msg_angles", config={"angle": "azimuth"},
             table={**points, "satellite_id": sat, "date": hours}, literals={"azimuth": msg_azimuth}),
        dict(id="reference_test_add_msg_angles_azimuth_with_config", filter="add_msg_angles",
             config={"satellite_id": "satid", "azimuth": "a", "angle": "azimuth"}, table={**points, "satid": sat, "date": hours},
             literals={"a": msg_azimuth}),
        dict(id="reference_test_add_msg_angles_zenith_default_config", filter="add_msg_angles", config={"angle": "zenith"},
             table={**points, "satellite_id": sat, "date": hours}, literals={"zenith": msg_zenith}),
        dict(id="reference_test_add_msg_angles_zenith_with_config", filter="add_msg_angles",
             config={"satellite_id": "satid", "zenith": "z", "angle": "zenith"}, table={**points, "satid": sat, "date": hours},
             literals={"z": msg_zenith}),
        dict(id="reference_test_add_msg_angles_both_default_config", filter="add_msg_angles", config={"angle": "both"},
             table={**points, "satellite_id": sat, "date": hours}, literals={"azimuth": msg_azimuth, "zenith": msg_zenith}),
        dict(id="reference_test_radiance_to_brightness_temperature", filter="radiance_to_brightness_temperature",
             config={"input_prefix": "obsvalue_rad_", "output_prefix": "obsvalue_rawbt_", "mode": "cris_fsr"},
             table={"obsvalue_rad_1": np.array([0.01, 0.1, 1.0])}, literals={"obsvalue_rawbt_1": [161.429057, 265.852062, 644.158476]}),
    ]
    return cases


def load_reference(src: str) -> dict:
    """``{filter name: class}`` of the reference's four filters, from its own files."""

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
    for name, members in stand_ins.items():
        module = types.ModuleType(name)
        module.__path__ = []  # a package, so that dotted imports below it resolve through sys.modules
        module.__dict__.update(members)
        sys.modules[name] = module
    tabular = os.path.join(src, "anemoi", "transform", "filters", "tabular")
    base = "anemoi.transform.filters.tabular"
    for name, path in ((f"{base}.support.utils", "support/utils.py"), (f"{base}.support.compute_forcings", "support/compute_forcings.py"),
                       (f"{base}.support.sat_view_angles", "support/sat_view_angles.py"), (f"{base}.add_forcings", "add_forcings.py"),
                       (f"{base}.add_azimuth", "add_azimuth.py"), (f"{base}.add_msg_angles", "add_msg_angles.py"),
                       (f"{base}.radiance_to_brightness_temperature", "radiance_to_brightness_temperature.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(tabular, path))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return registry.classes


def main() -> None:
    import pandas as pd

    import obs_rowops_restatement as R

    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("reference_src", help="the src/ directory of an anemoi-transform checkout")
    parser.add_argument("--out", default=R.GOLDEN)
    args = parser.parse_args()
    classes = load_reference(args.reference_src)
    cases = reference_cases() + [dict(id=name, filter=f, config=config, table=table) for name, f, config, table in R.seeded_cases()]
    records = []
    for case in cases:
        frame = classes[case["filter"]](**case["config"])(pd.DataFrame(case["table"]).copy())
        record = {"id": case["id"], "filter": case["filter"], "config": case["config"],
                  "table": {c: R.encode_column(v) for c, v in case["table"].items()},
                  "columns": list(frame.columns), "expected": {}}
        for c in frame.columns:  # only what the filter added or rewrote is stored: the other columns must come back as they went in
            spec = R.encode_column(frame[c].to_numpy())
            if spec != record["table"].get(c):
                record["expected"][c] = spec
        if "literals" in case:
            record["literals"], record["rtol"] = case["literals"], case.get("rtol", 1e-5)  # np.allclose's default where the test names none
            for column, values in case["literals"].items():
                assert np.allclose(frame[column].to_numpy(), values, rtol=record["rtol"]), (case["id"], column)
        records.append(record)
        print(f"{case['id']}: {len(frame)} rows, columns {list(frame.columns)}")
    with open(args.out, "w") as f:
        # one line per case keeps the file small and diffs readable
        f.write('{\n "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in records) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
