"""Grid-box statistics at the shapes they are for (O1280 -> O96 and 0.25 degree -> O96, 137 levels, float32 and float64): every statistic
against the grid-box-average gather on the same matrix, and against numpy on the host.

    python tools/box_statistics_bench.py --json profiles/box_statistics_bench.json

Per grid pair and type, in ONE process, interleaved round by round (device events around every call, every series warmed first), on the
same plan (``interp.box_average_rows`` built on the device, ``GatherPlan.from_matrix``) and the same buffers:
  - ``average`` / ``average_again``   ``GatherPlan.apply(x, out=y)``, the yardstick, timed as TWO series in every round: the difference
                                      of their medians is the run-to-run spread of this session;
  - ``maximum`` / ``minimum``         ``GatherPlan.reduce(x, s, out=y)``: no policy, non-negative weights — no weight word is read;
  - ``maximum_weights_read``          the same under ``missing="heaviest"``, which needs the weights (no NaN in the stack: the same values);
  - ``variance`` / ``standard-deviation``   two walks of the row;
  - ``mode_categorical``              the mode of a stack of classes 0 .. 20 that vary slowly over the sphere, all levels;
  - ``average_1`` / ``mode_categorical_1`` / ``maximum_1``   one level of it: the mode's real use, with its own yardstick.
Recorded: median / min / max per series, the ratio of each median to the yardstick's with the spread beside it, and the rate on the
gather's algorithmic bytes ``L B (U + Nt) + nnz (4 + B) + 4 (Nt + 1)`` (U: the source points some row names) as a fraction of the 8 TB/s
peak.  ``host``: numpy on this machine's CPU for ONE level (``np.fmax.reduceat`` / ``np.fmin.reduceat`` for the extremes, ``np.add.reduceat``
in two passes for the variance; median of 3), and that time scaled by the number of levels.  The mode has no numpy counterpart here:
not measured.  ``--pairs`` / ``--levels`` shrink the shapes for a rehearsal; the committed record is the default.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
from anemoi_transform_amd import interp  # noqa: E402
from anemoi_transform_amd.filters.regrid import as_gridspec  # noqa: E402
from anemoi_transform_amd.gather import GatherPlan  # noqa: E402
from anemoi_transform_amd.grids import lookup, row_structure  # noqa: E402
from anemoi_transform_amd.stack import Stack  # noqa: E402

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


def grid_arg(text: str):
    try:
        step = float(text)
        return [step, step]
    except ValueError:
        return text


def classes_on(grid: dict) -> np.ndarray:
    """Integers 0 .. 20 that vary slowly over the sphere, a few source cells in a thousand flipped to a neighbouring class."""
    lat, lon = np.radians(np.asarray(grid["latitudes"])), np.radians(np.asarray(grid["longitudes"]))
    smooth = 10.0 + 6.0 * np.sin(3.0 * lat) * np.cos(2.0 * lon) + 4.0 * np.cos(5.0 * lat + lon)
    rng = np.random.default_rng(5)
    return np.clip(np.rint(smooth) + (rng.random(lat.size) < 0.003), 0, 20)


def algorithmic_bytes(plan: GatherPlan, levels: int, B: int) -> int:
    used = int(np.unique(plan.indices).size)
    return levels * B * (used + plan.n_tgt) + len(plan.indices) * (4 + B) + 4 * (plan.n_tgt + 1)


def measure(plan: GatherPlan, classes: np.ndarray, levels: int, tdt, dev, reps: int, warm: int) -> dict:
    B = 4 if tdt == torch.float32 else 8
    gen = torch.Generator(device=dev).manual_seed(levels)
    x = Stack.empty(plan.n_src, levels, tdt, dev)
    x.data.copy_(280.0 + 50.0 * torch.rand(x.data.shape, device=dev, generator=gen, dtype=tdt))
    cat = Stack.empty(plan.n_src, levels, tdt, dev)
    cat.data.copy_(torch.from_numpy(classes).to(dev).to(tdt)[:, None].expand(-1, cat.data.shape[1]))
    cat1 = Stack.empty(plan.n_src, 1, tdt, dev)
    cat1.data.copy_(torch.from_numpy(classes).to(dev).to(tdt)[:, None].expand(-1, cat1.data.shape[1]))
    y = plan.apply(x)
    y1 = plan.apply(cat1)
    series = {
        "average": lambda: plan.apply(x, out=y),
        "average_again": lambda: plan.apply(x, out=y),
        "maximum": lambda: plan.reduce(x, "maximum", out=y),
        "minimum": lambda: plan.reduce(x, "minimum", out=y),
        "maximum_weights_read": lambda: plan.reduce(x, "maximum", missing="heaviest", out=y),
        "variance": lambda: plan.reduce(x, "variance", out=y),
        "standard-deviation": lambda: plan.reduce(x, "standard-deviation", out=y),
        "mode_categorical": lambda: plan.reduce(cat, "mode", out=y),
        "average_1": lambda: plan.apply(cat1, out=y1),
        "mode_categorical_1": lambda: plan.reduce(cat1, "mode", out=y1),
        "maximum_1": lambda: plan.reduce(cat1, "maximum", out=y1),
    }
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
    out = {name: spread(v) for name, v in ms.items()}
    a, b = out["average"]["median_ms"], out["average_again"]["median_ms"]
    base = 0.5 * (a + b)
    alg, alg1 = algorithmic_bytes(plan, levels, B), algorithmic_bytes(plan, 1, B)
    over = {f"{name}_over_average": out[name]["median_ms"] / base
            for name in ("maximum", "minimum", "maximum_weights_read", "variance", "standard-deviation", "mode_categorical")}
    over1 = {f"{name}_over_average_1": out[name]["median_ms"] / out["average_1"]["median_ms"] for name in ("mode_categorical_1", "maximum_1")}
    classes_met = int(torch.unique(plan.reduce(cat1, "mode").data[:, 0]).numel())
    return dict(series=out, algorithmic_bytes=alg, algorithmic_bytes_one_level=alg1, average_fraction_of_peak=alg / (base * 1e-3) / PEAK,
                maximum_fraction_of_peak=alg / (out["maximum"]["median_ms"] * 1e-3) / PEAK, average_run_to_run_spread=abs(a - b) / min(a, b),
                **over, **over1, distinct_modes_in_the_result=classes_met)


def host_times(plan: GatherPlan, values: np.ndarray, levels: int, T) -> dict:
    """numpy on the host, one level: the gathered sources reduced row by row (every row of a box-average matrix has entries)."""
    starts = plan.indptr[:-1].astype(np.intp)
    assert (np.diff(plan.indptr) > 0).all()
    x, w = values.astype(T), plan.data.astype(T)

    def variance():
        g = x[plan.indices]
        den = np.add.reduceat(w, starts)
        mean = np.add.reduceat(w * g, starts) / den
        d = g - np.repeat(mean, np.diff(plan.indptr))
        return np.add.reduceat(w * (d * d), starts) / den

    runs = {"maximum": lambda: np.fmax.reduceat(x[plan.indices], starts), "minimum": lambda: np.fmin.reduceat(x[plan.indices], starts),
            "variance": variance}
    out = {}
    for name, fn in runs.items():
        fn()
        took = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            took.append((time.perf_counter() - t0) * 1e3)
        one = float(np.median(took))
        out[name] = dict(one_level_ms=one, scaled_to_all_levels_ms=one * levels)
    return out


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "box_statistics_bench.json"))
    parser.add_argument("--pairs", default="O1280:O96,0.25:O96", help="source:target grid pairs, comma-separated")
    parser.add_argument("--levels", type=int, default=137)
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--warm", type=int, default=3)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing here falls back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    result = dict(device=torch.cuda.get_device_name(dev), levels=args.levels, peak_bytes_per_s=PEAK, reps=args.reps, warm=args.warm, pairs={})
    for pair in args.pairs.split(","):
        source, target = pair.split(":")
        src_grid = lookup(grid_arg(source))
        matrix = interp.box_average_rows(row_structure(as_gridspec(grid_arg(source))), row_structure(as_gridspec(grid_arg(target))), device=True)
        plan = GatherPlan.from_matrix(matrix)
        assert plan.kind == "csr", plan.kind
        lengths = np.diff(plan.indptr)
        classes = classes_on(src_grid)
        entry = dict(n_src=plan.n_src, n_tgt=plan.n_tgt, nnz=len(plan.indices), row_length_min=int(lengths.min()), row_length_max=int(lengths.max()),
                     row_length_mean=float(lengths.mean()), dtypes={}, host={})
        for tdt, T, tag in ((torch.float32, np.float32, "float32"), (torch.float64, np.float64, "float64")):
            entry["dtypes"][tag] = measure(plan, classes, args.levels, tdt, dev, args.reps, args.warm)
            print(pair, tag, json.dumps(entry["dtypes"][tag]), flush=True)
            torch.cuda.empty_cache()
            rng = np.random.default_rng(1)
            entry["host"][tag] = host_times(plan, 280.0 + 50.0 * rng.random(plan.n_src), args.levels, T)
            print(pair, tag, "host", json.dumps(entry["host"][tag]), flush=True)
        result["pairs"][pair] = entry
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
