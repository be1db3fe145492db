"""Missing-value-aware regridding at the headline shape (O1280 -> 0.25 degree, k = 4, 137 levels, float32 and float64): the renormalising
route against the plain gather it moves the bytes of, and against the composition a user had before it.

    python tools/regrid_missing_bench.py --json profiles/regrid_missing_bench.json

In ONE process, interleaved round by round (device events around every call, all shapes warmed first), on the same plan and buffers:
  - ``plain``        ``GatherPlan.apply(x, out=y)`` on the complete stack — timed as TWO series in every round: the difference of their
                     medians is the run-to-run spread of this session;
  - ``missing_0`` / ``missing_30`` / ``missing_100``
                     ``GatherPlan.apply(x, missing="all", out=y)`` with 0 %, 30 % and 100 % of the northern hemisphere's source points
                     NaN (all levels of a point);
  - ``missing_0_runtime_loop``
                     the 0 % case with a fifth, absent entry per row, which takes k = 4 off the compile-time ladder onto the run-time
                     loop of the same kernel: the A/B behind the ladder;
  - ``composition``  what the existing pieces offer, on the 30 % stack: impute NaN -> 0 (``pointwise_stack``), gather, gather of a 0 / 1
                     validity stack (built outside the timed window), divide (``torch.div``) — four launches, more than twice the bytes.
Recorded: median / min / max per series, ``missing_0 / plain`` with the spread beside it, and whether the composition is slower than
the new route.  The rate is on the plain gather's algorithmic bytes ``L B (U + Nt) + k Nt (4 + B)`` as a fraction of the 8 TB/s peak.
``--src`` / ``--tgt`` / ``--levels`` shrink the shape for a rehearsal; the committed record is the default shape.
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
from anemoi_transform_amd import interp, native  # noqa: E402
from anemoi_transform_amd.gather import GatherPlan  # noqa: E402
from anemoi_transform_amd.grids import lookup  # noqa: E402
from anemoi_transform_amd.stack import Stack  # noqa: E402

PEAK = 8e12
SHARES = (0, 30, 100)


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


def measure(plan: GatherPlan, north: np.ndarray, levels: int, tdt, dev, reps: int, warm: int) -> dict:
    B = 4 if tdt == torch.float32 else 8
    gen = torch.Generator(device=dev).manual_seed(levels)
    complete = Stack.empty(plan.n_src, levels, tdt, dev)
    complete.data.copy_(280.0 + 50.0 * torch.rand(complete.data.shape, device=dev, generator=gen, dtype=tdt))
    stacks = {}
    rng = np.random.default_rng(levels)
    for share in SHARES:
        gone = torch.from_numpy(north & (rng.random(plan.n_src) < share / 100.0)).to(dev)
        x = Stack.empty(plan.n_src, levels, tdt, dev)
        x.data.copy_(complete.data)
        x.data[gone] = float("nan")
        stacks[share] = x
    y = plan.apply(complete)
    loop_plan = GatherPlan(plan.n_src, plan.n_tgt, index=np.concatenate([plan.index, np.full((plan.n_tgt, 1), -1, dtype=np.int32)], axis=1),
                           weights=np.concatenate([plan.weights, np.zeros((plan.n_tgt, 1))], axis=1), padded=True)
    # the composition's buffers: the imputed stack, the validity stack (prebuilt), numerator and denominator
    holes = stacks[30]
    imputed, num, den = holes.new_like(), y.new_like(), y.new_like()
    validity = holes.new_like(zero=True)
    validity.data[:, :levels] = (~torch.isnan(holes.data[:, :levels])).to(tdt)
    impute = native.level_program([[(native.OP_IMPUTE_NAN, 0, 0.0, 0.0)] * levels], dev)

    def composition():
        native.pointwise_stack(holes.data, imputed.data, n_pts=holes.n_pts, n_lev=levels, x_pitch=holes.pitch, y_pitch=imputed.pitch,
                               layout=holes.layout, prog=impute, n_stage=1)
        plan.apply(imputed, out=num)
        plan.apply(validity, out=den)
        torch.div(num.data, den.data, out=num.data)

    series = {
        "plain": lambda: plan.apply(complete, out=y),
        "plain_again": lambda: plan.apply(complete, out=y),
        **{f"missing_{share}": (lambda s=share: plan.apply(stacks[s], missing="all", out=y)) for share in SHARES},
        "composition": composition,
        # the same four sources per row through the run-time loop: a fifth, absent entry (index -1) takes k off the compile-time ladder
        "missing_0_runtime_loop": lambda: loop_plan.apply(stacks[0], missing="all", out=y),
    }
    # what is timed computes the same thing: complete stack bit for bit, and the composition to rounding on the stack with holes
    plain = plan.apply(complete).data.clone()
    same_bits = bool(torch.equal(plan.apply(complete, missing="all").data[:, :levels].view(torch.int32 if B == 4 else torch.int64),
                                 plain[:, :levels].view(torch.int32 if B == 4 else torch.int64)))
    composition()
    new = plan.apply(holes, missing="all").data[:, :levels]
    old = num.data[:, :levels]
    both = ~torch.isnan(new)
    composition_agrees = bool(torch.equal(torch.isnan(new), torch.isnan(old)) and
                              torch.allclose(new[both], old[both], rtol=1e-5 if B == 4 else 1e-13, atol=0.0))
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
    used = int(np.unique(plan.index[plan.index >= 0]).size)
    alg = levels * B * (used + plan.n_tgt) + plan.k * plan.n_tgt * (4 + B)
    a, b = out["plain"]["median_ms"], out["plain_again"]["median_ms"]
    base = 0.5 * (a + b)
    run_to_run = abs(a - b) / min(a, b)
    ratios = {f"missing_{share}_over_plain": out[f"missing_{share}"]["median_ms"] / base for share in SHARES}
    return dict(
        series=out, algorithmic_bytes=alg, plain_fraction_of_peak=alg / (base * 1e-3) / PEAK,
        missing_0_fraction_of_peak=alg / (out["missing_0"]["median_ms"] * 1e-3) / PEAK,
        plain_run_to_run_spread=run_to_run, **ratios,
        missing_0_within_three_spreads=bool(abs(ratios["missing_0_over_plain"] - 1.0) <= 3.0 * run_to_run),
        runtime_loop_over_compile_time_k=out["missing_0_runtime_loop"]["median_ms"] / out["missing_0"]["median_ms"],
        composition_over_missing_30=out["composition"]["median_ms"] / out["missing_30"]["median_ms"],
        complete_stack_equals_plain_bit_for_bit=same_bits, composition_agrees_to_rounding=composition_agrees,
    )


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "regrid_missing_bench.json"))
    parser.add_argument("--src", default="O1280")
    parser.add_argument("--tgt", default="0.25")
    parser.add_argument("--levels", type=int, default=137)
    parser.add_argument("--k", type=int, default=4)
    parser.add_argument("--reps", type=int, default=30)
    parser.add_argument("--warm", type=int, default=3)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing here falls back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    src_grid, tgt_grid = lookup(grid_arg(args.src)), lookup(grid_arg(args.tgt))
    idx, w = interp.knn_inverse_distance(src_grid, tgt_grid, k=args.k)
    plan = GatherPlan(len(src_grid["latitudes"]), len(tgt_grid["latitudes"]), index=idx, weights=w)
    north = np.asarray(src_grid["latitudes"]) > 0.0
    result = dict(device=torch.cuda.get_device_name(dev), source=args.src, target=args.tgt, k=plan.k, levels=args.levels, n_src=plan.n_src,
                  n_tgt=plan.n_tgt, peak_bytes_per_s=PEAK, reps=args.reps, nan_shares_of_the_northern_hemisphere_percent=list(SHARES), dtypes={})
    for tdt, tag in ((torch.float32, "float32"), (torch.float64, "float64")):
        result["dtypes"][tag] = measure(plan, north, args.levels, tdt, dev, args.reps, args.warm)
        print(tag, json.dumps(result["dtypes"][tag]), flush=True)
        torch.cuda.empty_cache()
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
