"""Column integrals at the shapes they are for: O1280 x 137 model levels — total column water vapour and the two components of the
integrated vapour transport over the whole column — and 0.25 degrees x 13 pressure levels — the same three outputs and, in a second
call, the mean of ``q`` between 850 and 500 hPa — float32 and float64, both layouts.

    python tools/integral_bench.py --json profiles/integral_bench.json

Per shape and type, in ONE process, interleaved round by round (device events around every call, every series warmed first), on the
same buffers:
  - ``columns`` / ``columns_again``   ``vertical.integrate_columns`` on column stacks — the LDS-tile kernel — timed as TWO series in every
                                      round: the difference of their medians is the run-to-run spread of this session;
  - ``fields``                        the same call on field-major stacks that are already there: one lane per (point, bound);
  - ``relayout_fields``               what serving a column stack by the field-major kernel costs: relayout, that kernel, relayout back;
  - ``torch``                         the same statement with torch on the same device: the weights of every (point, level) in float64,
                                      then ``(x * dp).sum``;
  - ``copy``                          a plain device copy that reads and writes the ALGORITHMIC bytes — the variables and sp read, the
                                      results written: the byte bound of any design.
Recorded: median / min / max per series, the kernel over the copy and over torch, the rate on the algorithmic bytes as a fraction of the
8 TB/s HBM peak, whether the layouts give the same bits and how far torch's result is from the kernel's.  NOT measured here: kernel time
apart from the launch (no profiler run), counters, more than one device, shapes other than those named.  ``--small`` shrinks the grids
for a rehearsal; the committed record is the default.
"""

from __future__ import annotations

import argparse
import json
import math
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
from anemoi_transform_amd.vertical import G, integrate_columns  # noqa: E402

PEAK = 8e12
TERMS = [(0, -1), (0, 1), (0, 2)]  # q, q u, q v
PL_HPA = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
# (grid, levtype, levels): every case is TERMS over the whole column; "pl" adds a second call, the mean of q over 850 - 500 hPa
SHAPES = [("o1280", "ml", 137), ("0.25", "pl", 13)]


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


def torch_weights(sp: torch.Tensor, top: float, bottom: float, A=None, B=None, P=None) -> torch.Tensor:
    """The weights of include/atx_integral.h with torch, float64 ``[n_pts, n_lev]``."""
    s = sp.double()[:, None]
    if P is None:
        lo, hi = A[None, :-1] + B[None, :-1] * s, A[None, 1:] + B[None, 1:] * s
        return (hi.clamp(max=bottom) - lo.clamp(min=top)).clamp(min=0.0)
    above = P[None, :] <= s
    pj, pn = P[None, :-1], P[None, 1:]
    a, c = pj.clamp(min=top), pn.clamp(max=bottom)
    length = (c - a).clamp(min=0.0) * above[:, 1:]
    r = ((a + c) / 2 - pj) / (pn - pj)
    w = torch.zeros((sp.numel(), P.numel()), dtype=torch.float64, device=sp.device)
    w[:, :-1] += length * (1.0 - r)
    w[:, 1:] += length * r
    last = above.clone()
    last[:, :-1] &= ~above[:, 1:]
    return w + (s.clamp(max=bottom) - P[None, :].clamp(min=top)).clamp(min=0.0) * last


def torch_statement(x: torch.Tensor, sp: torch.Tensor, terms, top: float, bottom: float, mean: bool, n_lev: int, **table) -> torch.Tensor:
    """``x [n_pts, n_var * n_lev]`` -> ``[n_pts, n_term]``: ``(x * dp).sum`` over the levels, by ``g`` or by the weight sum."""
    w = torch_weights(sp, top, bottom, **table)
    col = lambda v: x[:, v * n_lev:(v + 1) * n_lev].double()  # noqa: E731
    sums = [(w * (col(v1) if v2 < 0 else col(v1) * col(v2))).sum(dim=1) for v1, v2 in terms]
    return (torch.stack(sums, dim=1) / (w.sum(dim=1, keepdim=True) if mean else G)).to(x.dtype)


def measure(n_pts: int, levtype: str, n_lev: int, tdt, dev, reps: int, warm: int) -> dict:
    itemsize = 4 if tdt == torch.float32 else 8
    gen = torch.Generator(device=dev).manual_seed(itemsize * 100 + n_lev)
    sp = (60000.0 + 44000.0 * torch.rand(n_pts, device=dev, generator=gen, dtype=torch.float64)).to(tdt)
    x = Stack.empty(n_pts, 3 * n_lev, tdt, dev, COLUMNS, zero=True)
    for v, (scale, mean) in enumerate(((4e-3, 5e-3), (20.0, 3.0), (20.0, 0.0))):  # q, u, v
        x.data[:, v * n_lev:(v + 1) * n_lev] = mean + scale * (torch.rand((n_pts, n_lev), device=dev, generator=gen, dtype=tdt) - 0.5)
    xf = x.to_layout(FIELDS)
    if levtype == "ml":
        eta = torch.arange(n_lev + 1, dtype=torch.float64, device=dev) / n_lev
        table = dict(A=20000.0 * eta * (1.0 - eta), B=((eta - 0.3).clamp(min=0.0) / 0.7) ** 2)
        calls = [(TERMS, None, "integral")]
    else:
        table = dict(levels_pa=torch.tensor(PL_HPA, dtype=torch.float64, device=dev) * 100.0)
        calls = [(TERMS, None, "integral"), ([(0, -1)], [(50000.0, 85000.0)], "mean")]
    torch_table = {("P" if k == "levels_pa" else k): v for k, v in table.items()}
    n_out = sum(len(terms) for terms, _, _ in calls)
    alg = (3 * n_lev + 1 + n_out) * n_pts * itemsize
    half = torch.empty(alg // 2, dtype=torch.uint8, device=dev), torch.empty(alg // 2, dtype=torch.uint8, device=dev)
    xt = x.data[:, :3 * n_lev]

    def kernel(stack):
        return [integrate_columns(stack, sp, terms, bounds, n_var=3, kind=kind, **table) for terms, bounds, kind in calls]

    def with_torch():
        return [torch_statement(xt, sp, terms, *(bounds[0] if bounds else (0.0, math.inf)), kind == "mean", n_lev, **torch_table) for terms, bounds, kind in calls]

    series = {
        "columns": lambda: kernel(x),
        "columns_again": lambda: kernel(x),
        "fields": lambda: kernel(xf),
        "relayout_fields": lambda: [y.to_layout(COLUMNS) for y in kernel(x.to_layout(FIELDS))],
        "torch": with_torch,
        "copy": lambda: half[1].copy_(half[0]),
    }
    got = run_series(series, reps, warm)
    ys, yfs, yts = kernel(x), [y.to_layout(COLUMNS) for y in kernel(xf)], with_torch()
    bits = torch.int32 if itemsize == 4 else torch.int64
    rows = [len(terms) for terms, _, _ in calls]
    a, b = got["columns"]["median_ms"], got["columns_again"]["median_ms"]
    call = 0.5 * (a + b)
    return dict(calls=[dict(terms=terms, bounds_pa=bounds, kind=kind) for terms, bounds, kind in calls], series=got, algorithmic_bytes=alg,
                columns_fraction_of_peak=alg / (call * 1e-3) / PEAK, fields_fraction_of_peak=alg / (got["fields"]["median_ms"] * 1e-3) / PEAK,
                copy_fraction_of_peak=alg / (got["copy"]["median_ms"] * 1e-3) / PEAK, columns_run_to_run_spread=abs(a - b) / min(a, b),
                columns_over_copy=call / got["copy"]["median_ms"], torch_over_columns=got["torch"]["median_ms"] / call,
                fields_over_columns=got["fields"]["median_ms"] / call, relayout_fields_over_columns=got["relayout_fields"]["median_ms"] / call,
                layouts_give_the_same_bits=all(bool(torch.equal(y.data[:, :n].view(bits), yf.data[:, :n].view(bits))) for y, yf, n in zip(ys, yfs, rows)),
                torch_max_difference_over_max=max(float((yt.double() - y.data[:, :n].double()).abs().max() / y.data[:, :n].double().abs().max())
                                                  for y, yt, n in zip(ys, yts, rows)))


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "integral_bench.json"))
    parser.add_argument("--small", action="store_true", help="10 degree and o32 grids: a rehearsal of the script, not a measurement")
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--warm", type=int, default=2)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing here falls back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    grids = {"0.25": "10.0" if args.small else "0.25", "o1280": "o32" if args.small else "o1280"}
    result = dict(device=torch.cuda.get_device_name(dev), peak_bytes_per_s=PEAK, reps=args.reps, warm=args.warm, block=8, grids=grids,
                  not_measured="kernel time apart from the launch, counters, more than one device, other shapes", shapes={})
    for grid, levtype, n_lev in SHAPES:
        name = grids[grid]
        n_pts = len(lookup([float(name), float(name)] if name[0].isdigit() else name)["latitudes"])
        for tdt, tag in ((torch.float32, "float32"), (torch.float64, "float64")):
            key = f"{name}_x_{n_lev}_{levtype}_{tag}"
            result["shapes"][key] = dict(n_pts=n_pts, **measure(n_pts, levtype, n_lev, tdt, dev, args.reps, args.warm))
            print(key, json.dumps(result["shapes"][key]), flush=True)
            torch.cuda.empty_cache()
            with open(args.json, "w") as f:  # after every shape: a run cut short leaves what it measured
                json.dump(result, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
