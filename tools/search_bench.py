"""The column search at the shapes it is for: O1280 x 137 model levels and 0.25 degrees x 13 pressure levels, the ``t`` = 273.15 K crossing
from the ground and the maximum of a wind-speed column, each with ``z``, ``u``, ``v`` out, float32 and float64.

    python tools/search_bench.py --json profiles/search_bench.json

Per shape, search and type, in ONE process, interleaved round by round (device events around every call, every series warmed first), on
the same buffers:
  - ``columns`` / ``columns_again``   ``vertical.search_columns`` on column stacks — the LDS-tile kernel with the wave-cooperative search —
                                      timed as TWO series in every round: the difference of their medians is the run-to-run spread;
  - ``fields``                        the same call on field-major stacks that are already there: one lane per (point, target);
  - ``relayout_fields``               a column stack served through the field-major kernel: both stacks relaid, the call, the result
                                      relaid back — what ``SEARCH_COLUMNS_ROUTE = "fields"`` would cost a filter;
  - ``torch``                         the same statement with torch on the same device: compare, ``cummax`` / ``argmax`` and ``gather`` over the
                                      ``[n_pts, n_lev]`` mask, the weight and the result in float64;
  - ``copy``                          a plain device copy that reads and writes the ALGORITHMIC bytes — the variables and the search column
                                      read, the result rows written: the byte bound of any design.
Recorded: median / min / max per series, the kernel over the copy and over torch, whether the layouts give the same bits and how far
torch's result is from the kernel's.  NOT measured here: kernel time apart from the launch (no profiler run), counters, more than one
device, ``count``, ``level_values``, a lane per (point, target) walking its column in LDS (the alternative to the ballot that the kernel's
header comment names), shapes other than those named.  ``--small`` shrinks the grids for a rehearsal; the committed record is the default.
"""

from __future__ import annotations

import argparse
import gc
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
from anemoi_transform_amd.vertical import search_columns  # noqa: E402

PEAK = 8e12
N_VAR = 3  # z, u, v
SHAPES = [("o1280", 137), ("0.25", 13)]  # (grid, levels)
SEARCHES = {"t_273.15_from_the_ground": dict(direction="backward", mode="any"), "wind_speed_maximum": dict(direction="forward", mode="max")}
T0 = 273.15


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
            gc.collect()  # (between calls, outside every timed region: a relaid O1280 x 137 stack is 20 GiB, and nothing else frees it in time)
    torch.cuda.synchronize()
    ms = {name: [] for name in names}
    for r in range(reps):
        for i in range(len(names)):  # a rotating order: no series always follows the same neighbour
            name = names[(i + r) % len(names)]
            ms[name].append(timed(series[name]))
            gc.collect()
    return {name: spread(v) for name, v in ms.items()}


def torch_statement(x: torch.Tensor, s: torch.Tensor, n_var: int, direction: str, mode: str) -> torch.Tensor:
    """include/atx_search.h with torch: ``x [n_pts, n_var * n_lev]``, ``s [n_pts, n_lev]`` -> ``[n_pts, n_var]`` (one target, T0)."""
    n_pts, n = s.shape
    e = s.double() if direction == "forward" else s.double().flip(1)
    nan = torch.full((n_pts, 1), float("nan"), dtype=torch.float64, device=s.device)
    if mode == "max":
        k = torch.where(e.isnan(), torch.full_like(e, float("-inf")), e).argmax(dim=1, keepdim=True)
        found, w, k1 = ~e.isnan().all(dim=1, keepdim=True), torch.zeros_like(nan), k
    else:
        here, following = e[:, :-1], e[:, 1:]
        hit = ((here <= T0) & (T0 < following)) | ((here >= T0) & (T0 > following))
        found, k = hit.any(dim=1, keepdim=True), hit.int().argmax(dim=1, keepdim=True)
        k1 = k + 1
        w = (T0 - e.gather(1, k)) / (e.gather(1, k1) - e.gather(1, k))
    out = []
    for v in range(n_var):
        xv = x[:, v * n:(v + 1) * n].double()
        xv = xv if direction == "forward" else xv.flip(1)
        xa, xb = xv.gather(1, k), xv.gather(1, k1)
        out.append(torch.where(found, xa + w * (xb - xa) if mode != "max" else xa, nan))
    return torch.cat(out, dim=1).to(x.dtype)


def measure(n_pts: int, n_lev: int, search: dict, tdt, dev, reps: int, warm: int) -> dict:
    itemsize = 4 if tdt == torch.float32 else 8
    gen = torch.Generator(device=dev).manual_seed(itemsize * 100 + n_lev)
    s = Stack.empty(n_pts, n_lev, tdt, dev, COLUMNS, zero=True)
    if search["mode"] == "max":  # a wind speed with a jet somewhere and noise on it
        s.data[:, :n_lev] = (40.0 * torch.rand((n_pts, n_lev), device=dev, generator=gen, dtype=torch.float64)).to(tdt)
    else:  # a temperature that falls with height (row 0 is the top) with noise large enough for inversions around the freezing level
        lapse = torch.linspace(215.0, 305.0, n_lev, device=dev, dtype=torch.float64)
        s.data[:, :n_lev] = (lapse[None, :] + 3.0 * torch.randn((n_pts, n_lev), device=dev, generator=gen, dtype=torch.float64)).to(tdt)
    x = Stack.empty(n_pts, N_VAR * n_lev, tdt, dev, COLUMNS, zero=True)
    for v in range(N_VAR):
        x.data[:, v * n_lev:(v + 1) * n_lev] = -30.0 + 60.0 * torch.rand((n_pts, n_lev), device=dev, generator=gen, dtype=tdt)
    xf, sf = x.to_layout(FIELDS), s.to_layout(FIELDS)
    targets = torch.tensor([T0], dtype=torch.float64, device=dev)
    alg = ((N_VAR + 1) * n_lev + N_VAR) * n_pts * itemsize
    half = torch.empty(alg // 2, dtype=torch.uint8, device=dev), torch.empty(alg // 2, dtype=torch.uint8, device=dev)
    xt, st = x.data[:, :N_VAR * n_lev], s.data[:, :n_lev]
    call = lambda a, b: search_columns(a, b, targets, n_var=N_VAR, **search)[0]  # noqa: E731
    series = {
        "columns": lambda: call(x, s),
        "columns_again": lambda: call(x, s),
        "fields": lambda: call(xf, sf),
        "relayout_fields": lambda: call(x.to_layout(FIELDS), s.to_layout(FIELDS)).to_layout(COLUMNS),
        "torch": lambda: torch_statement(xt, st, N_VAR, **search),
        "copy": lambda: half[1].copy_(half[0]),
    }
    got = run_series(series, reps, warm)
    y, yf, yt = call(x, s), call(xf, sf).to_layout(COLUMNS), torch_statement(xt, st, N_VAR, **search)
    bits = torch.int32 if itemsize == 4 else torch.int64
    a, b = got["columns"]["median_ms"], got["columns_again"]["median_ms"]
    kernel = 0.5 * (a + b)
    found = ~y.data[:, :N_VAR].isnan().any(dim=1)
    return dict(series=got, algorithmic_bytes=alg, columns_fraction_of_peak=alg / (kernel * 1e-3) / PEAK,
                fields_fraction_of_peak=alg / (got["fields"]["median_ms"] * 1e-3) / PEAK, copy_fraction_of_peak=alg / (got["copy"]["median_ms"] * 1e-3) / PEAK,
                columns_run_to_run_spread=abs(a - b) / min(a, b), columns_over_copy=kernel / got["copy"]["median_ms"],
                fields_over_copy=got["fields"]["median_ms"] / got["copy"]["median_ms"], torch_over_columns=got["torch"]["median_ms"] / kernel,
                fields_over_columns=got["fields"]["median_ms"] / kernel, relayout_fields_over_columns=got["relayout_fields"]["median_ms"] / kernel,
                layouts_give_the_same_bits=bool(torch.equal(y.data[:, :N_VAR].view(bits), yf.data[:, :N_VAR].view(bits))),
                torch_max_abs_difference=float((yt.double() - y.data[:, :N_VAR].double())[found].abs().max()) if bool(found.any()) else None,
                torch_agrees_on_what_is_found=bool(torch.equal(found, ~yt.isnan().any(dim=1))), points_with_an_answer=int(found.sum()))


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "search_bench.json"))
    parser.add_argument("--small", action="store_true", help="10 degree and o32 grids: a rehearsal of the script, not a measurement")
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--warm", type=int, default=2)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing here falls back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    grids = {"0.25": "10.0" if args.small else "0.25", "o1280": "o32" if args.small else "o1280"}
    result = dict(device=torch.cuda.get_device_name(dev), peak_bytes_per_s=PEAK, reps=args.reps, warm=args.warm, variables_out=N_VAR, grids=grids,
                  not_measured="kernel time apart from the launch, counters, more than one device, count, level_values, a lane per (point, target) "
                               "walking its column in LDS, other shapes", shapes={})
    for grid, n_lev in SHAPES:
        name = grids[grid]
        n_pts = len(lookup([float(name), float(name)] if name[0].isdigit() else name)["latitudes"])
        for label, search in SEARCHES.items():
            for tdt, tag in ((torch.float32, "float32"), (torch.float64, "float64")):
                key = f"{name}_x_{n_lev}_levels_{label}_{tag}"
                result["shapes"][key] = dict(n_pts=n_pts, **measure(n_pts, n_lev, search, tdt, dev, args.reps, args.warm))
                print(key, json.dumps(result["shapes"][key]), flush=True)
                torch.cuda.empty_cache()
                with open(args.json, "w") as f:  # after every shape: a run cut short leaves what it measured
                    json.dump(result, f, indent=1)
                    f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
