"""Model levels to pressure levels at the shape it is for: O1280 x 137 model levels -> 13 pressure levels, 1 and 5 variables, float32
and float64, both layouts.

    python tools/levels_bench.py --json profiles/levels_bench.json

Per (variables, type), in ONE process, interleaved round by round (device events around every call, every series warmed first), on the
same buffers:
  - ``columns`` / ``columns_again``   ``vertical.interpolate_levels`` on the column stack — the LDS-tile kernel — timed as TWO series in
                                      every round: the difference of their medians is the run-to-run spread of this session;
  - ``fields``                        the same call on a field-major stack that is already there: the one-lane-per-(point, target) kernel;
  - ``relayout_then_fields``          the column stack converted to field-major (``atx_relayout``), then the field-major kernel: what a
                                      caller with a column stack pays for that route;
  - ``relayout_fields_relayout``      and the 13 levels converted back, which is what the ``ml_to_pl`` filter would do on that route;
  - ``torch``                         the same statement in torch on the same device: p_full for every point, ``searchsorted``, ``gather``,
                                      ``lerp`` (float64 arithmetic, as the kernel's).
Recorded: median / min / max per series and the rate on the algorithmic bytes — ``n_var n_lev N B`` read, ``N B`` of surface pressure,
``n_var n_tgt N B`` written — as a fraction of the 8 TB/s HBM peak; the largest difference between the kernel's and torch's results.
``chain``: ``ml_to_pl | regrid`` against ``regrid | ml_to_pl`` for the O1280 -> 0.25 degree k = 4 matrix of the headline (one variable,
float32): interpolate 137 -> 13 levels and gather 13, or gather 137 levels and the surface pressure and interpolate on the target grid.
``--grid`` / ``--levels`` shrink the shapes for a rehearsal; the committed record is the default.
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
from anemoi_transform_amd.gather import GatherPlan  # noqa: E402
from anemoi_transform_amd.grids import lookup  # noqa: E402
from anemoi_transform_amd.interp import knn_inverse_distance  # noqa: E402
from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack  # noqa: E402
from anemoi_transform_amd.vertical import interpolate_levels  # noqa: E402

PEAK = 8e12
TARGETS_HPA = (1000, 925, 850, 700, 600, 500, 400, 300, 250, 200, 150, 100, 50)


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


def torch_statement(x: torch.Tensor, sp: torch.Tensor, A: torch.Tensor, B: torch.Tensor, P: torch.Tensor, n_var: int, n_lev: int) -> torch.Tensor:
    """The statement of include/atx_levels.h ("linear", "nearest") on a column stack's tensor, in torch: ``[n_pts, n_var * n_tgt]``."""
    n_pts, n_tgt = x.shape[0], P.numel()
    s = sp.to(torch.float64)[:, None]
    ph = A[None, :] + B[None, :] * s
    pf = (ph[:, :-1] + ph[:, 1:]) / 2
    targets = P[None, :].expand(n_pts, -1).contiguous()
    i = torch.searchsorted(pf, targets, right=True)
    a, b = (i - 1).clamp_(0, n_lev - 1), i.clamp(0, n_lev - 1)
    pa, pb = pf.gather(1, a), pf.gather(1, b)
    w = torch.where(a == b, torch.zeros_like(pa), (targets - pa) / (pb - pa))
    out = torch.empty((n_pts, n_var * n_tgt), dtype=x.dtype, device=x.device)
    for v in range(n_var):
        xv = x[:, v * n_lev:(v + 1) * n_lev]
        out[:, v * n_tgt:(v + 1) * n_tgt] = torch.lerp(xv.gather(1, a).to(torch.float64), xv.gather(1, b).to(torch.float64), w).to(x.dtype)
    return out


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


def measure(n_pts: int, n_var: int, n_lev: int, tdt, dev, reps: int, warm: int) -> dict:
    itemsize = 4 if tdt == torch.float32 else 8
    gen = torch.Generator(device=dev).manual_seed(n_var * 1000 + itemsize)
    A, B = hybrid_table(n_lev, dev)
    sp = (50000.0 + 55000.0 * torch.rand(n_pts, device=dev, generator=gen, dtype=torch.float64)).to(tdt)
    targets = [100.0 * v for v in TARGETS_HPA]
    P = torch.tensor(targets, dtype=torch.float64, device=dev)
    x = Stack.empty(n_pts, n_var * n_lev, tdt, dev, COLUMNS, zero=True)
    x.data[:, : n_var * n_lev] = 220.0 + 80.0 * torch.rand((n_pts, n_var * n_lev), device=dev, generator=gen, dtype=tdt)
    xf = x.to_layout(FIELDS)
    kw = dict(n_var=n_var)
    series = {
        "columns": lambda: interpolate_levels(x, sp, A, B, P, **kw),
        "columns_again": lambda: interpolate_levels(x, sp, A, B, P, **kw),
        "fields": lambda: interpolate_levels(xf, sp, A, B, P, **kw),
        "relayout_then_fields": lambda: interpolate_levels(x.to_layout(FIELDS), sp, A, B, P, **kw),
        "relayout_fields_relayout": lambda: interpolate_levels(x.to_layout(FIELDS), sp, A, B, P, **kw).to_layout(COLUMNS),
        "torch": lambda: torch_statement(x.data, sp, A, B, P, n_var, n_lev),
    }
    out = run_series(series, reps, warm)
    y = interpolate_levels(x, sp, A, B, P, **kw)
    yf = interpolate_levels(xf, sp, A, B, P, **kw).to_layout(COLUMNS)
    same_bits = bool(torch.equal(y.data[:, : y.n_lev].view(torch.int32 if itemsize == 4 else torch.int64),
                                 yf.data[:, : yf.n_lev].view(torch.int32 if itemsize == 4 else torch.int64)))
    apart = float((y.data[:, : y.n_lev].to(torch.float64) - torch_statement(x.data, sp, A, B, P, n_var, n_lev).to(torch.float64)).abs().max())
    alg = n_var * n_lev * n_pts * itemsize + n_pts * itemsize + n_var * len(targets) * n_pts * itemsize
    a, b = out["columns"]["median_ms"], out["columns_again"]["median_ms"]
    base = 0.5 * (a + b)
    rates = {f"{name}_fraction_of_peak": alg / (out[name]["median_ms"] * 1e-3) / PEAK for name in ("fields", "relayout_then_fields",
                                                                                                  "relayout_fields_relayout", "torch")}
    return dict(series=out, algorithmic_bytes=alg, columns_fraction_of_peak=alg / (base * 1e-3) / PEAK, **rates,
                columns_run_to_run_spread=abs(a - b) / min(a, b), torch_over_columns=out["torch"]["median_ms"] / base,
                relayout_then_fields_over_columns=out["relayout_then_fields"]["median_ms"] / base,
                relayout_fields_relayout_over_columns=out["relayout_fields_relayout"]["median_ms"] / base,
                fields_over_columns=out["fields"]["median_ms"] / base, layouts_give_the_same_bits=same_bits, largest_difference_from_torch=apart)


def chain(src_name: str, tgt_name: str, n_lev: int, dev, reps: int, warm: int) -> dict:
    """``ml_to_pl | regrid`` against ``regrid | ml_to_pl``, one float32 variable, the headline's k = 4 matrix."""
    src_grid, tgt_grid = lookup(src_name), lookup(tgt_name)
    n_src, n_tgt = len(src_grid["latitudes"]), len(tgt_grid["latitudes"])
    idx, w = knn_inverse_distance(src_grid, tgt_grid, k=4, device=True, ties="index")
    plan = GatherPlan(n_src, n_tgt, index=idx, weights=w)
    gen = torch.Generator(device=dev).manual_seed(4)
    A, B = hybrid_table(n_lev, dev)
    targets = torch.tensor([100.0 * v for v in TARGETS_HPA], dtype=torch.float64, device=dev)
    x = Stack.empty(n_src, n_lev, torch.float32, dev, COLUMNS, zero=True)
    x.data[:, :n_lev] = 220.0 + 80.0 * torch.rand((n_src, n_lev), device=dev, generator=gen, dtype=torch.float32)
    sp = Stack.empty(n_src, 1, torch.float32, dev, COLUMNS)
    sp.data.copy_((50000.0 + 55000.0 * torch.rand((n_src, 1), device=dev, generator=gen, dtype=torch.float64)).to(torch.float32))
    series = {
        "ml_to_pl_then_regrid": lambda: plan.apply(interpolate_levels(x, sp.data[:, 0], A, B, targets)),
        "regrid_then_ml_to_pl": lambda: interpolate_levels(plan.apply(x), plan.apply(sp).data[:, 0], A, B, targets),
        "regrid_137_levels_alone": lambda: plan.apply(x),
    }
    out = run_series(series, reps, warm)
    return dict(n_src=n_src, n_tgt=n_tgt, k=4, series=out,
                regrid_first_over_levels_first=out["regrid_then_ml_to_pl"]["median_ms"] / out["ml_to_pl_then_regrid"]["median_ms"])


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "levels_bench.json"))
    parser.add_argument("--grid", default="o1280")
    parser.add_argument("--target-grid", default="0.25")
    parser.add_argument("--levels", type=int, default=137)
    parser.add_argument("--variables", default="1,5")
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--warm", type=int, default=2)
    parser.add_argument("--no-chain", action="store_true")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing here falls back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n_pts = len(lookup(args.grid)["latitudes"])
    result = dict(device=torch.cuda.get_device_name(dev), grid=args.grid, n_pts=n_pts, levels=args.levels, targets_hpa=list(TARGETS_HPA),
                  peak_bytes_per_s=PEAK, reps=args.reps, warm=args.warm, shapes={})
    for n_var in (int(v) for v in args.variables.split(",")):
        for tdt, tag in ((torch.float32, "float32"), (torch.float64, "float64")):
            key = f"{n_var}-variables-{tag}"
            result["shapes"][key] = measure(n_pts, n_var, args.levels, tdt, dev, args.reps, args.warm)
            print(key, json.dumps(result["shapes"][key]), flush=True)
            torch.cuda.empty_cache()
    if not args.no_chain:
        result["chain"] = chain(args.grid, args.target_grid, args.levels, dev, args.reps, args.warm)
        print("chain", json.dumps(result["chain"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
