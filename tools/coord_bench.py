"""Interpolation on a coordinate field at the shapes it is for: 0.25 degrees x 13 pressure levels to {10, 100, 200} m above the ground
for one and four variables, and O1280 x 137 model levels with ``z`` on them to 3 and 13 heights, float32 and float64, both layouts.

    python tools/coord_bench.py --json profiles/coord_bench.json

Per shape and type, in ONE process, interleaved round by round (device events around every call, every series warmed first), on the
same buffers:
  - ``columns`` / ``columns_again``   ``vertical.interpolate_on_coordinate`` on column stacks — the LDS-tile kernel — timed as TWO series in
                                      every round: the difference of their medians is the run-to-run spread of this session;
  - ``fields``                        the same call on field-major stacks that are already there: one lane per (point, target);
  - ``torch``                         the same statement with torch on the same device: ``searchsorted`` on the column put in ascending
                                      order, ``gather`` of the bracket, the weight and the result in float64 (policy "nearest");
  - ``copy``                          a plain device copy that reads and writes the ALGORITHMIC bytes — the variables, the coordinate and
                                      the offset read, n_var x n_tgt rows and the bad bytes written: the byte bound of any design.
Recorded: median / min / max per series, the kernel over the copy and over torch, the rate on the algorithmic bytes as a fraction of
the 8 TB/s HBM peak, whether the layouts give the same bits and how far torch's result is from the kernel's.  NOT measured here: kernel
time apart from the launch (no profiler run), counters, more than one device, the floor, shapes other than those named.  ``--small``
shrinks the grids for a rehearsal; the committed record is the default.
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
from anemoi_transform_amd.vertical import G, interpolate_on_coordinate  # noqa: E402

PEAK = 8e12
HEIGHTS = {3: [10.0, 100.0, 200.0], 13: [2.0, 10.0, 50.0, 100.0, 200.0, 500.0, 1000.0, 2000.0, 3000.0, 5000.0, 10000.0, 20000.0, 40000.0]}
# (grid, levels, variables, targets)
SHAPES = [("0.25", 13, 1, 3), ("0.25", 13, 4, 3), ("o1280", 137, 1, 3), ("o1280", 137, 1, 13)]


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


def torch_statement(x: torch.Tensor, c: torch.Tensor, targets: torch.Tensor, offset: torch.Tensor, n_var: int) -> torch.Tensor:
    """include/atx_coord.h with torch, policy "nearest": ``x [n_pts, n_var * n_lev]``, ``c [n_pts, n_lev]`` -> ``[n_pts, n_var * n_tgt]``."""
    n_pts, n = c.shape
    c64 = c.double()
    steps = c64[:, 1:] - c64[:, :-1]
    up, down = (steps > 0).all(dim=1), (steps < 0).all(dim=1)
    e = torch.where(up[:, None], c64, c64.flip(1))
    T = targets[None, :] + offset.double()[:, None]
    i = torch.searchsorted(e, T, right=True)
    a, b = (i - 1).clamp(0, n - 1), i.clamp(0, n - 1)
    w = (T - e.gather(1, a)) / (e.gather(1, b) - e.gather(1, a))
    copy = (i == 0) | (i == n)
    out = []
    for v in range(n_var):
        xv = x[:, v * n:(v + 1) * n].double()
        xv = torch.where(up[:, None], xv, xv.flip(1))
        xa, xb = xv.gather(1, a), xv.gather(1, b)
        y = torch.where(copy, xa, xa + w * (xb - xa))
        out.append(torch.where((up | down)[:, None], y, torch.full_like(y, float("nan"))))
    return torch.cat(out, dim=1).to(x.dtype)


def measure(n_pts: int, n_lev: int, n_var: int, n_tgt: int, tdt, dev, reps: int, warm: int) -> dict:
    itemsize = 4 if tdt == torch.float32 else 8
    gen = torch.Generator(device=dev).manual_seed(itemsize * 100 + n_lev + n_var)
    zs = (30000.0 * torch.rand(n_pts, device=dev, generator=gen, dtype=torch.float64) - 300.0).to(tdt)
    coord = Stack.empty(n_pts, n_lev, tdt, dev, COLUMNS, zero=True)
    layers = 100.0 + 4000.0 * torch.rand((n_pts, n_lev), device=dev, generator=gen, dtype=torch.float64)
    coord.data[:, :n_lev] = (zs.double()[:, None] + layers.cumsum(dim=1).flip(1)).to(tdt)  # falls towards the ground, which comes last
    del layers
    x = Stack.empty(n_pts, n_var * n_lev, tdt, dev, COLUMNS, zero=True)
    for v in range(n_var):
        x.data[:, v * n_lev:(v + 1) * n_lev] = -30.0 + 60.0 * torch.rand((n_pts, n_lev), device=dev, generator=gen, dtype=tdt)
    xf, cf = x.to_layout(FIELDS), coord.to_layout(FIELDS)
    targets = torch.tensor(HEIGHTS[n_tgt], dtype=torch.float64, device=dev) * G
    rows = n_var * n_tgt
    alg = ((n_var + 1) * n_lev + 1 + rows) * n_pts * itemsize + n_pts
    half = torch.empty(alg // 2, dtype=torch.uint8, device=dev), torch.empty(alg // 2, dtype=torch.uint8, device=dev)
    xt, ct = x.data[:, :n_var * n_lev], coord.data[:, :n_lev]
    series = {
        "columns": lambda: interpolate_on_coordinate(x, coord, targets, n_var=n_var, offset=zs),
        "columns_again": lambda: interpolate_on_coordinate(x, coord, targets, n_var=n_var, offset=zs),
        "fields": lambda: interpolate_on_coordinate(xf, cf, targets, n_var=n_var, offset=zs),
        "torch": lambda: torch_statement(xt, ct, targets, zs, n_var),
        "copy": lambda: half[1].copy_(half[0]),
    }
    got = run_series(series, reps, warm)
    y, bad = interpolate_on_coordinate(x, coord, targets, n_var=n_var, offset=zs)
    yf = interpolate_on_coordinate(xf, cf, targets, n_var=n_var, offset=zs)[0].to_layout(COLUMNS)
    yt = torch_statement(xt, ct, targets, zs, n_var)
    bits = torch.int32 if itemsize == 4 else torch.int64
    a, b = got["columns"]["median_ms"], got["columns_again"]["median_ms"]
    kernel = 0.5 * (a + b)
    return dict(heights_m=HEIGHTS[n_tgt], series=got, algorithmic_bytes=alg, columns_fraction_of_peak=alg / (kernel * 1e-3) / PEAK,
                fields_fraction_of_peak=alg / (got["fields"]["median_ms"] * 1e-3) / PEAK, copy_fraction_of_peak=alg / (got["copy"]["median_ms"] * 1e-3) / PEAK,
                columns_run_to_run_spread=abs(a - b) / min(a, b), columns_over_copy=kernel / got["copy"]["median_ms"],
                torch_over_columns=got["torch"]["median_ms"] / kernel, fields_over_columns=got["fields"]["median_ms"] / kernel,
                layouts_give_the_same_bits=bool(torch.equal(y.data[:, :rows].view(bits), yf.data[:, :rows].view(bits))),
                torch_max_abs_difference=float((yt.double() - y.data[:, :rows].double()).abs().max()), bad_points=int(bad.sum()))


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "coord_bench.json"))
    parser.add_argument("--small", action="store_true", help="10 degree and o32 grids: a rehearsal of the script, not a measurement")
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--warm", type=int, default=2)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing here falls back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    grids = {"0.25": "10.0" if args.small else "0.25", "o1280": "o32" if args.small else "o1280"}
    result = dict(device=torch.cuda.get_device_name(dev), peak_bytes_per_s=PEAK, reps=args.reps, warm=args.warm, reference="ground (offset = zs)",
                  grids=grids, not_measured="kernel time apart from the launch, counters, more than one device, the floor, other shapes", shapes={})
    for grid, n_lev, n_var, n_tgt in SHAPES:
        name = grids[grid]
        n_pts = len(lookup([float(name), float(name)] if name[0].isdigit() else name)["latitudes"])
        for tdt, tag in ((torch.float32, "float32"), (torch.float64, "float64")):
            key = f"{name}_x_{n_lev}_levels_{n_var}_variables_{n_tgt}_targets_{tag}"
            result["shapes"][key] = dict(n_pts=n_pts, **measure(n_pts, n_lev, n_var, n_tgt, tdt, dev, args.reps, args.warm))
            print(key, json.dumps(result["shapes"][key]), flush=True)
            torch.cuda.empty_cache()
            with open(args.json, "w") as f:  # after every shape: a run cut short leaves what it measured
                json.dump(result, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
