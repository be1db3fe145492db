"""Geopotential on model levels at the shape it is for: O1280 x 137 model levels, float32 and float64, both layouts.

    python tools/geopotential_bench.py --json profiles/geopotential_bench.json

Per type, in ONE process, interleaved round by round (device events around every call, every series warmed first), on the same buffers:
  - ``columns`` / ``columns_again``   ``vertical.geopotential_on_model_levels`` on two column stacks — the LDS-tile kernel — timed as TWO
                                      series in every round: the difference of their medians is the run-to-run spread of this session;
  - ``fields``                        the same call on field-major stacks that are already there: the one-lane-per-point kernel;
  - ``relayout_fields_relayout``      both column stacks converted to field-major (``atx_relayout``), the field-major kernel, and the
                                      result converted back: what the filter would pay on that route (GEOPOTENTIAL_COLUMNS_ROUTE);
  - ``pressure_at_height``            ``atx_pressure_at_height_stack`` on the same t and q column stacks (100 m): the older hydrostatic
                                      kernel, one lane per column in global memory, as a yardstick — it reads the same two stacks and
                                      writes one value per point.
Recorded: median / min / max per series and the rate on the algorithmic bytes — two stacks, ``sp`` and ``zs`` read, one stack written — as
a fraction of the 8 TB/s HBM peak (a byte bound: each (point, level) also costs one float64 logarithm and two float64 divisions, which
are not counted).  NOT measured here: kernel time apart from the launch (no profiler run), counters, more than one device, and shapes
other than the one named.  ``--grid`` / ``--levels`` shrink the shape for a rehearsal; the committed record is the default.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
from anemoi_transform_amd import native  # noqa: E402
from anemoi_transform_amd.grids import lookup  # noqa: E402
from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack  # noqa: E402
from anemoi_transform_amd.vertical import geopotential_on_model_levels  # noqa: E402

PEAK = 8e12


def spread(ms: list) -> dict:
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=len(ms))


def timed(fn) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def hybrid_table(n_lev: int, dev) -> tuple[torch.Tensor, torch.Tensor]:
    """A smooth table with the ground as its last half level: B = eta^2, A = 20000 eta (1 - eta)."""
    eta = torch.arange(n_lev + 1, dtype=torch.float64, device=dev) / n_lev
    return 20000.0 * eta * (1.0 - eta), eta * eta


def run_series(series: dict, reps: int, warm: int) -> dict:
    names = list(series)
    for _ in range(warm):
        for name in names:
            series[name]()
    torch.cuda.synchronize()
    ms = {name: [] for name in names}
    for r in range(reps):
        for i in range(len(names)):  # a rotating order: no series always follows the same neighbour
            name = names[(i + r) % len(names)]
            ms[name].append(timed(series[name]))
    return {name: spread(v) for name, v in ms.items()}


def measure(n_pts: int, n_lev: int, tdt, dev, reps: int, warm: int) -> dict:
    itemsize = 4 if tdt == torch.float32 else 8
    gen = torch.Generator(device=dev).manual_seed(itemsize)
    A, B = hybrid_table(n_lev, dev)
    sp = (50000.0 + 55000.0 * torch.rand(n_pts, device=dev, generator=gen, dtype=torch.float64)).to(tdt)
    zs = (-500.0 + 30000.0 * torch.rand(n_pts, device=dev, generator=gen, dtype=torch.float64)).to(tdt)
    t, q = Stack.empty(n_pts, n_lev, tdt, dev, COLUMNS, zero=True), Stack.empty(n_pts, n_lev, tdt, dev, COLUMNS, zero=True)
    t.data[:, :n_lev] = 220.0 + 80.0 * torch.rand((n_pts, n_lev), device=dev, generator=gen, dtype=tdt)
    q.data[:, :n_lev] = 0.02 * torch.rand((n_pts, n_lev), device=dev, generator=gen, dtype=tdt)
    tf, qf = t.to_layout(FIELDS), q.to_layout(FIELDS)
    p_out = torch.empty(n_pts, dtype=tdt, device=dev)
    series = {
        "columns": lambda: geopotential_on_model_levels(t, q, sp, zs, A, B),
        "columns_again": lambda: geopotential_on_model_levels(t, q, sp, zs, A, B),
        "fields": lambda: geopotential_on_model_levels(tf, qf, sp, zs, A, B),
        "relayout_fields_relayout": lambda: geopotential_on_model_levels(t.to_layout(FIELDS), q.to_layout(FIELDS), sp, zs, A, B).to_layout(COLUMNS),
        "pressure_at_height": lambda: native.pressure_at_height_stack(t.data, q.data, sp, A, B, p_out, n_pts=n_pts, n_lev=n_lev, pitch=t.pitch,
                                                                      layout=COLUMNS, height=100.0),
    }
    out = run_series(series, reps, warm)
    bits = torch.int32 if itemsize == 4 else torch.int64
    y = geopotential_on_model_levels(t, q, sp, zs, A, B)
    yf = geopotential_on_model_levels(tf, qf, sp, zs, A, B).to_layout(COLUMNS)
    same_bits = bool(torch.equal(y.data[:, :n_lev].view(bits), yf.data[:, :n_lev].view(bits)))
    alg = 3 * n_lev * n_pts * itemsize + 2 * n_pts * itemsize
    a, b = out["columns"]["median_ms"], out["columns_again"]["median_ms"]
    base = 0.5 * (a + b)
    rates = {f"{name}_fraction_of_peak": alg / (out[name]["median_ms"] * 1e-3) / PEAK for name in ("fields", "relayout_fields_relayout")}
    return dict(series=out, algorithmic_bytes=alg, columns_fraction_of_peak=alg / (base * 1e-3) / PEAK, **rates,
                columns_run_to_run_spread=abs(a - b) / min(a, b), fields_over_columns=out["fields"]["median_ms"] / base,
                relayout_fields_relayout_over_columns=out["relayout_fields_relayout"]["median_ms"] / base,
                pressure_at_height_over_columns=out["pressure_at_height"]["median_ms"] / base, layouts_give_the_same_bits=same_bits,
                lowest_and_top_level_mean=[float(y.data[:, n_lev - 1].double().mean()), float(y.data[:, 0].double().mean())])


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "geopotential_bench.json"))
    parser.add_argument("--grid", default="o1280")
    parser.add_argument("--levels", type=int, default=137)
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--warm", type=int, default=2)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing here falls back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n_pts = len(lookup(args.grid)["latitudes"])
    result = dict(device=torch.cuda.get_device_name(dev), grid=args.grid, n_pts=n_pts, levels=args.levels, peak_bytes_per_s=PEAK, reps=args.reps,
                  warm=args.warm, not_measured="kernel time apart from the launch, counters, more than one device, other shapes", shapes={})
    for tdt, tag in ((torch.float32, "float32"), (torch.float64, "float64")):
        result["shapes"][tag] = measure(n_pts, args.levels, tdt, dev, args.reps, args.warm)
        print(tag, json.dumps(result["shapes"][tag]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
