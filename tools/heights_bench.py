"""Model levels to height levels at the shape it is for: O1280 x 137 model levels, float32 and float64, 1 and 4 variables, the targets
{10, 100, 200} m and thirteen heights, above the ground, both layouts.

    python tools/heights_bench.py --json profiles/heights_bench.json

Per type, number of variables and number of targets, in ONE process, interleaved round by round (device events around every call, every
series warmed first), on the same buffers:
  - ``columns`` / ``columns_again``   ``vertical.interpolate_to_heights`` on column stacks — the fused LDS-tile kernel — timed as TWO series
                                      in every round: the difference of their medians is the run-to-run spread of this session;
  - ``fields``                        the same call on field-major stacks that are already there: one lane per (point, target), which
                                      walks the column twice — the plain kernel, whose goal is the same bits, not speed;
  - ``geopotential``                  ``vertical.geopotential_on_model_levels`` on the same t and q column stacks: 137 levels of z written;
  - ``levels_log``                    ``vertical.interpolate_levels`` (log p) on the same variables, to as many pressure targets.
``geopotential`` + ``levels_log`` is the floor of any UNFUSED height-level design: it would have to write z, and then interpolate on a
per-point coordinate, which costs at least what interpolating on a coordinate shared by every point does.  Recorded: median / min / max
per series, the sum of the two, the fused kernel over that sum, and the rate on the algorithmic bytes — the variables, t, q and sp read,
n_var x n_tgt rows written — as a fraction of the 8 TB/s HBM peak (a byte bound: each (point, level) also costs one float64 logarithm
and two float64 divisions, which are not counted).  NOT measured here: kernel time apart from the launch (no profiler run), counters, more
than one device, the sea reference (one more vector read) and shapes other than those named.  ``--grid`` / ``--levels`` shrink the shape
for a rehearsal; the committed record is the default.
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
from anemoi_transform_amd.grids import lookup  # noqa: E402
from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack  # noqa: E402
from anemoi_transform_amd.vertical import geopotential_on_model_levels, interpolate_levels, interpolate_to_heights  # noqa: E402

PEAK = 8e12
HEIGHTS = {3: [10.0, 100.0, 200.0], 13: [2.0, 10.0, 50.0, 100.0, 200.0, 500.0, 1000.0, 2000.0, 3000.0, 5000.0, 10000.0, 20000.0, 40000.0]}
PRESSURES = {3: [100000.0, 92500.0, 85000.0],
             13: [100000.0, 92500.0, 85000.0, 70000.0, 60000.0, 50000.0, 40000.0, 30000.0, 25000.0, 20000.0, 15000.0, 10000.0, 5000.0]}


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


def filled(n_pts: int, n_rows: int, tdt, dev, gen, low: float, width: float) -> Stack:
    stack = Stack.empty(n_pts, n_rows, tdt, dev, COLUMNS, zero=True)
    for a in range(0, n_rows, 137):  # in slabs: the generator's own buffer stays small next to the stack
        b = min(n_rows, a + 137)
        stack.data[:, a:b] = low + width * torch.rand((n_pts, b - a), device=dev, generator=gen, dtype=tdt)
    return stack


def measure(n_pts: int, n_lev: int, n_var: int, tdt, dev, reps: int, warm: int) -> dict:
    itemsize = 4 if tdt == torch.float32 else 8
    gen = torch.Generator(device=dev).manual_seed(itemsize * 10 + n_var)
    A, B = hybrid_table(n_lev, dev)
    sp = (50000.0 + 55000.0 * torch.rand(n_pts, device=dev, generator=gen, dtype=torch.float64)).to(tdt)
    t, q = filled(n_pts, n_lev, tdt, dev, gen, 220.0, 80.0), filled(n_pts, n_lev, tdt, dev, gen, 0.0, 0.02)
    x = filled(n_pts, n_var * n_lev, tdt, dev, gen, -30.0, 60.0)
    tf, qf, xf = t.to_layout(FIELDS), q.to_layout(FIELDS), x.to_layout(FIELDS)
    bits = torch.int32 if itemsize == 4 else torch.int64
    out = {}
    for n_tgt, heights in HEIGHTS.items():
        pressures = PRESSURES[n_tgt]
        series = {
            "columns": lambda: interpolate_to_heights(x, t, q, sp, None, A, B, heights, n_var=n_var),
            "columns_again": lambda: interpolate_to_heights(x, t, q, sp, None, A, B, heights, n_var=n_var),
            "fields": lambda: interpolate_to_heights(xf, tf, qf, sp, None, A, B, heights, n_var=n_var),
            "geopotential": lambda: geopotential_on_model_levels(t, q, sp, None, A, B),
            "levels_log": lambda: interpolate_levels(x, sp, A, B, pressures, n_var=n_var, coordinate="log"),
        }
        got = run_series(series, reps, warm)
        y = interpolate_to_heights(x, t, q, sp, None, A, B, heights, n_var=n_var)
        yf = interpolate_to_heights(xf, tf, qf, sp, None, A, B, heights, n_var=n_var).to_layout(COLUMNS)
        rows = n_var * n_tgt
        same_bits = bool(torch.equal(y.data[:, :rows].view(bits), yf.data[:, :rows].view(bits)))
        alg = ((n_var + 2) * n_lev + 1 + rows) * n_pts * itemsize
        a, b = got["columns"]["median_ms"], got["columns_again"]["median_ms"]
        fused = 0.5 * (a + b)
        unfused = got["geopotential"]["median_ms"] + got["levels_log"]["median_ms"]
        out[f"{n_tgt}_targets"] = dict(
            heights_m=heights, series=got, algorithmic_bytes=alg, columns_fraction_of_peak=alg / (fused * 1e-3) / PEAK,
            fields_fraction_of_peak=alg / (got["fields"]["median_ms"] * 1e-3) / PEAK, columns_run_to_run_spread=abs(a - b) / min(a, b),
            fields_over_columns=got["fields"]["median_ms"] / fused, geopotential_plus_levels_log_ms=unfused, fused_over_geopotential_plus_levels_log=fused / unfused,
            layouts_give_the_same_bits=same_bits, first_and_last_target_mean=[float(y.data[:, 0].double().mean()), float(y.data[:, n_tgt - 1].double().mean())])
        print(n_var, "variables", n_tgt, "targets", json.dumps(out[f"{n_tgt}_targets"]), flush=True)
    return out


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "heights_bench.json"))
    parser.add_argument("--grid", default="o1280")
    parser.add_argument("--levels", type=int, default=137)
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--warm", type=int, default=2)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing here falls back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n_pts = len(lookup(args.grid)["latitudes"])
    result = dict(device=torch.cuda.get_device_name(dev), grid=args.grid, n_pts=n_pts, levels=args.levels, reference="ground", peak_bytes_per_s=PEAK,
                  reps=args.reps, warm=args.warm, not_measured="kernel time apart from the launch, counters, more than one device, the sea reference, other shapes",
                  shapes={})
    for tdt, tag in ((torch.float32, "float32"), (torch.float64, "float64")):
        for n_var in (1, 4):
            result["shapes"][f"{tag}_{n_var}_variables"] = measure(n_pts, args.levels, n_var, tdt, dev, args.reps, args.warm)
            torch.cuda.empty_cache()
        with open(args.json, "w") as f:  # after every type: a run cut short leaves what it measured
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
