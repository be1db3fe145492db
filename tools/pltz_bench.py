"""t and z on pressure levels (and msl) at the shape they are for: O1280 x 137 model levels to 13 pressure levels, float32 and float64,
both layouts.

    python tools/pltz_bench.py --json profiles/pltz_bench.json

Per type, in ONE process, interleaved round by round (device events around every call, every series warmed first), on the same buffers:
  - ``columns`` / ``columns_again``   ``vertical.t_z_on_pressure_levels`` on column stacks — the fused LDS-tile kernel — timed as TWO series
                                      in every round: the difference of their medians is the run-to-run spread of this session;
  - ``fields``                        the same call on field-major stacks that are already there: one lane per point, which walks the
                                      column once per interior target — the plain kernel, whose goal is the same bits, not speed;
  - ``geopotential``                  ``vertical.geopotential_on_model_levels`` on the same t and q column stacks: 137 levels of z written;
  - ``levels_two``                    ``vertical.interpolate_levels`` of TWO variables (t and that z) to the same pressure levels.
``geopotential`` + ``levels_two`` is the route this kernel replaces for t and z (it gives no extrapolation and no msl).  Recorded: median /
min / max per series, the sum of the two, the fused kernel over that sum, and the rate on the algorithmic bytes — t, q, sp and zs read,
2 x 13 + 1 rows written — as a fraction of the 8 TB/s HBM peak (a byte bound: each (point, level) also costs one float64 logarithm and two
float64 divisions, which are not counted).  NOT measured here: kernel time apart from the launch (no profiler run), counters, more than
one device, the log coordinate and shapes other than those named.  ``--grid`` / ``--levels`` shrink the shape for a rehearsal; the
committed record is the default.
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
from anemoi_transform_amd.vertical import geopotential_on_model_levels, interpolate_levels, t_z_on_pressure_levels  # noqa: E402

PEAK = 8e12
PRESSURES = [100000.0, 92500.0, 85000.0, 70000.0, 60000.0, 50000.0, 40000.0, 30000.0, 25000.0, 20000.0, 15000.0, 10000.0, 5000.0]


def spread(ms: list) -> dict:
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=len(ms))


def timed(fn) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


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
    eta = torch.arange(n_lev + 1, dtype=torch.float64, device=dev) / n_lev  # a smooth table with the ground as its last half level
    A, B = 20000.0 * eta * (1.0 - eta), eta * eta
    rand = lambda n, low, width: (low + width * torch.rand(n, device=dev, generator=gen, dtype=torch.float64)).to(tdt)  # noqa: E731
    sp, zs = rand(n_pts, 50000.0, 55000.0), rand(n_pts, -500.0, 40000.0)  # 22 % of the outputs are under the ground

    def filled(n_rows: int, low: float, width: float) -> Stack:
        stack = Stack.empty(n_pts, n_rows, tdt, dev, COLUMNS, zero=True)
        for a in range(0, n_rows, n_lev):  # in slabs: the generator's own buffer stays small next to the stack
            stack.data[:, a:a + n_lev] = low + width * torch.rand((n_pts, n_lev), device=dev, generator=gen, dtype=tdt)
        return stack

    t, q, two = filled(n_lev, 220.0, 80.0), filled(n_lev, 0.0, 0.02), filled(2 * n_lev, 220.0, 80.0)  # two: the t and the z of the unfused route
    tf, qf = t.to_layout(FIELDS), q.to_layout(FIELDS)
    series = {
        "columns": lambda: t_z_on_pressure_levels(t, q, sp, zs, A, B, PRESSURES),
        "columns_again": lambda: t_z_on_pressure_levels(t, q, sp, zs, A, B, PRESSURES),
        "fields": lambda: t_z_on_pressure_levels(tf, qf, sp, zs, A, B, PRESSURES),
        "geopotential": lambda: geopotential_on_model_levels(t, q, sp, zs, A, B),
        "levels_two": lambda: interpolate_levels(two, sp, A, B, PRESSURES, n_var=2),
    }
    got = run_series(series, reps, warm)
    rows = 2 * len(PRESSURES) + 1
    bits = torch.int32 if itemsize == 4 else torch.int64
    y = t_z_on_pressure_levels(t, q, sp, zs, A, B, PRESSURES)
    yf = t_z_on_pressure_levels(tf, qf, sp, zs, A, B, PRESSURES).to_layout(COLUMNS)
    alg = (2 * n_lev + 2 + rows) * n_pts * itemsize
    a, b = got["columns"]["median_ms"], got["columns_again"]["median_ms"]
    fused, unfused = 0.5 * (a + b), got["geopotential"]["median_ms"] + got["levels_two"]["median_ms"]
    out = dict(pressures_pa=PRESSURES, series=got, algorithmic_bytes=alg, columns_fraction_of_peak=alg / (fused * 1e-3) / PEAK,
               fields_fraction_of_peak=alg / (got["fields"]["median_ms"] * 1e-3) / PEAK, columns_run_to_run_spread=abs(a - b) / min(a, b),
               fields_over_columns=got["fields"]["median_ms"] / fused, geopotential_plus_levels_two_ms=unfused, fused_over_geopotential_plus_levels_two=fused / unfused,
               layouts_give_the_same_bits=bool(torch.equal(y.data[:, :rows].view(bits), yf.data[:, :rows].view(bits))),
               fraction_of_outputs_under_the_ground=float((torch.tensor(PRESSURES, device=dev)[None, :] > sp.double()[:, None]).double().mean()),
               mean_t1000_z1000_msl=[float(y.data[:, 0].double().mean()), float(y.data[:, len(PRESSURES)].double().mean()), float(y.data[:, rows - 1].double().mean())])
    print(json.dumps(out), flush=True)
    return out


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "pltz_bench.json"))
    parser.add_argument("--grid", default="o1280")
    parser.add_argument("--levels", type=int, default=137)
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--warm", type=int, default=2)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing here falls back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n_pts = len(lookup(args.grid)["latitudes"])
    result = dict(device=torch.cuda.get_device_name(dev), grid=args.grid, n_pts=n_pts, levels=args.levels, coordinate="linear", msl=True,
                  peak_bytes_per_s=PEAK, reps=args.reps, warm=args.warm,
                  not_measured="kernel time apart from the launch, counters, more than one device, the log coordinate, other shapes", shapes={})
    for tdt, tag in ((torch.float32, "float32"), (torch.float64, "float64")):
        result["shapes"][tag] = measure(n_pts, args.levels, tdt, dev, args.reps, args.warm)
        torch.cuda.empty_cache()
        with open(args.json, "w") as f:  # after every type: a run cut short leaves what it measured
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
