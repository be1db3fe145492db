"""Grid-box-average regridding at production sizes: how long the matrix takes to build on the host and on the device, and how fast
the general CSR gather applies it.

    python tools/box_average_bench.py --json profiles/box_average_bench.json

For O1280 -> O96, 0.25 degree -> O96 and O2560 -> 0.25 degree it records
  - nnz and the range of row lengths;
  - the host build (``interp.box_average_rows(device=False)``, one run, wall clock);
  - the device build — count + scan + fill on tables already in HBM — timed with device events after warming, ``--reps`` runs, the
    median with the smallest and the largest; and ``device=True`` as a caller sees it (upload, build, download), wall clock;
  - that the two builds are equal bit for bit;
  - the gather of the resulting plan (what ``regrid(method="grid-box-average")`` runs) on a 137-level column stack in float64 and
    float32: the median time and the rate on the algorithmic bytes ``L B (U + Nt) + nnz (4 + B)``, as a fraction of the 8 TB/s peak;
and, for comparison, the stand-in row that tools/kernel_bench.py tracks (unweighted box average O1280 -> 1 degree, general CSR).
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
from anemoi_transform_amd import interp, native_plan  # noqa: E402
from anemoi_transform_amd.gather import GatherPlan  # noqa: E402
from anemoi_transform_amd.grids import lookup, row_structure  # noqa: E402
from anemoi_transform_amd.stack import Stack  # noqa: E402

PEAK = 8e12
PAIRS = [("O1280", "O96"), ([0.25, 0.25], "O96"), ("O2560", [0.25, 0.25])]


def spread(ms: list[float]) -> dict:
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=len(ms))


def device_events(fn, reps: int, warm: int = 3) -> dict:
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    return spread(ms)


def device_build_timed(src_rows, tgt_rows, dev, reps: int) -> dict:
    tables = [native_plan.RowTable(*(torch.from_numpy(a).to(dev) for a in interp.box_row_table(rows)), n_points=int(np.sum(rows[1])))
              for rows in (src_rows, tgt_rows)]
    n_tgt = tables[1].n_points
    count = torch.empty(n_tgt, dtype=torch.int64, device=dev)
    native_plan.box_average_count(tables[0], tables[1], count)
    nnz = int(count.sum().item())
    indptr = torch.zeros(n_tgt + 1, dtype=torch.int32, device=dev)
    indices = torch.empty(nnz, dtype=torch.int32, device=dev)
    data = torch.empty(nnz, dtype=torch.float64, device=dev)

    def build():  # no host synchronisation inside: nnz is known from the warm-up, as it is to a caller who rebuilds a plan
        native_plan.box_average_count(tables[0], tables[1], count)
        indptr[1:] = torch.cumsum(count, dim=0).to(torch.int32)
        native_plan.box_average_fill(tables[0], tables[1], indptr, indices, data)

    parts = dict(
        count=device_events(lambda: native_plan.box_average_count(tables[0], tables[1], count), reps),
        fill=device_events(lambda: native_plan.box_average_fill(tables[0], tables[1], indptr, indices, data), reps),
    )
    return dict(count_scan_fill=device_events(build, reps), **parts)


def gather_rows(plan: GatherPlan, n_src: int, n_tgt: int, nnz: int, used: int, levels: int, dev, reps: int) -> dict:
    out = {}
    for tdt, B, tag in ((torch.float64, 8, "float64"), (torch.float32, 4, "float32")):
        gen = torch.Generator(device=dev).manual_seed(levels)
        x = Stack.empty(n_src, levels, tdt, dev)
        x.data.copy_(torch.rand(x.data.shape, device=dev, generator=gen, dtype=tdt))
        y = plan.apply(x)
        timing = device_events(lambda: plan.apply(x, out=y), reps)
        alg = levels * B * (used + n_tgt) + nnz * (4 + B)
        rate = alg / (timing["median_ms"] * 1e-3)
        out[tag] = dict(**timing, algorithmic_bytes=alg, tb_per_s=rate / 1e12, fraction_of_peak=rate / PEAK, plan_kind=plan.kind)
        del x, y
    return out


def stand_in(levels: int, dev, reps: int) -> dict:
    """tools/kernel_bench.py's row "regrid_csr box average O1280->1deg": every 1-degree cell averages the O1280 points inside it."""
    src_grid, one = lookup("O1280"), lookup([1.0, 1.0])
    n_src, n_one = len(src_grid["latitudes"]), len(one["latitudes"])
    cell = (np.rint(90.0 - src_grid["latitudes"]).astype(np.int64) * 360 + np.mod(np.rint(src_grid["longitudes"]).astype(np.int64), 360))
    order = np.argsort(cell, kind="stable")
    counts = np.bincount(cell, minlength=n_one)
    indptr = np.concatenate([[0], np.cumsum(counts)])
    plan = GatherPlan(n_src, n_one, csr=((1.0 / np.maximum(counts, 1))[cell[order]], order.astype(np.int32), indptr))
    return dict(nnz=n_src, n_src=n_src, n_tgt=n_one, gather=gather_rows(plan, n_src, n_one, n_src, n_src, levels, dev, reps))


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "box_average_bench.json"))
    parser.add_argument("--levels", type=int, default=137)
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--pairs", type=int, nargs="*", default=None, help="indices into the three pairs (default: all)")
    parser.add_argument("--no-stand-in", action="store_true")
    args = parser.parse_args()
    assert torch.cuda.is_available() and args.reps >= 20
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    result = dict(device=torch.cuda.get_device_name(dev), levels=args.levels, peak_bytes_per_s=PEAK, pairs=[])
    for n, (src, tgt) in enumerate(PAIRS):
        if args.pairs is not None and n not in args.pairs:
            continue
        src_rows, tgt_rows = row_structure(src), row_structure(tgt)
        t0 = time.perf_counter()
        host = interp.box_average_rows(src_rows, tgt_rows, device=False)
        host_s = time.perf_counter() - t0
        interp.box_average_rows(src_rows, tgt_rows, device=True)  # warm: library load, allocator
        t0 = time.perf_counter()
        built = interp.box_average_rows(src_rows, tgt_rows, device=True)
        device_call_s = time.perf_counter() - t0
        equal = all(np.array_equal(host[k], built[k]) and host[k].dtype == built[k].dtype for k in host)
        lengths = np.diff(host["matrix_indptr"].astype(np.int64))
        n_tgt, n_src = (int(v) for v in host["matrix_shape"])
        nnz, used = len(host["matrix_indices"]), int(np.unique(host["matrix_indices"]).size)
        tgt_grid = lookup(tgt)
        from anemoi_transform_amd.filters.regrid import _ordered

        plan = _ordered(GatherPlan.from_matrix(host), tgt_grid)  # the plan of regrid(method="grid-box-average")
        row = dict(
            source=str(src), target=str(tgt), n_src=n_src, n_tgt=n_tgt, nnz=nnz, source_columns_used=used,
            row_length=dict(min=int(lengths.min()), max=int(lengths.max()), mean=float(lengths.mean())),
            host_build_s=host_s, device_call_s=device_call_s, device_equals_host_bit_for_bit=bool(equal),
            device_build=device_build_timed(src_rows, tgt_rows, dev, args.reps),
            targets_ordered=plan.order is not None,
            gather=gather_rows(plan, n_src, n_tgt, nnz, used, args.levels, dev, args.reps),
        )
        row["host_over_device_build"] = host_s / (row["device_build"]["count_scan_fill"]["median_ms"] * 1e-3)
        result["pairs"].append(row)
        print(json.dumps(row), flush=True)
        del host, built, plan
        torch.cuda.empty_cache()
    if not args.no_stand_in:
        result["stand_in_box_average_O1280_to_1deg"] = stand_in(args.levels, dev, args.reps)
        print(json.dumps(result["stand_in_box_average_O1280_to_1deg"]), flush=True)
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
