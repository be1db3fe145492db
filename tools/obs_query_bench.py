#!/usr/bin/env python3
"""``filter_query`` on one MI355X at --rows resident rows, with the first query of the reference's docstring,

    varno in [1,2,3,4,7,59] and pressure in [85000, 92500, 100000]

over a table of device tensors (int64 ``varno``, float64 ``pressure``, six more float64 columns): the whole ``forward`` (compile, the
int64 -> float64 pass over ``varno``, the expression launch, the scan of the chunk counts, the positions launch and the gather of all
eight columns), the row selection alone (``obs.query_rows``), the expression launch alone and the positions launch alone; beside them
``DataFrame.query`` of the same table on this host's CPU.

    python tools/obs_query_bench.py --out profiles/obs_query_bench.json [--rows 10000000]

Device variants are timed with device events, one call at a time, INTERLEAVED over --rounds rounds after a warm-up of every one of them;
the median is reported with the smallest and largest reading.  An event pair around a whole ``forward`` also counts the host's share
(the compiler, the allocations, the one synchronising read of the kept count).  pandas: one warm-up call, the median of three.  The
filter's rows are checked against pandas' before anything is timed."""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import __graft_entry__ as graft  # noqa: E402
from obs_qc_bench import host_ms, interleaved  # noqa: E402

QUERY = "varno in [1,2,3,4,7,59] and pressure in [85000, 92500, 100000]"


def build_table(n: int) -> dict:
    rng = np.random.default_rng(n)
    table = {"varno": rng.choice([1, 2, 3, 4, 7, 29, 59, 111], n).astype(np.int64),
             "pressure": rng.choice([100000.0, 92500.0, 85000.0, 70000.0, 50000.0, 30000.0], n)}
    for name in ("fg_depar_t_0", "fg_depar_q_0", "fg_depar_z_0", "obsvalue", "latitude", "longitude"):
        table[name] = rng.standard_normal(n)
    return table


def main() -> None:
    import pandas as pd

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    graft.load_package()
    from anemoi_transform_amd import native, obs
    from anemoi_transform_amd.filters import create_filter_by_name

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.rows
    host = build_table(n)
    table = {c: torch.from_numpy(v).to(dev) for c, v in host.items()}
    frame = pd.DataFrame(host)
    f = create_filter_by_name("filter_query", query=QUERY)
    program = obs.compile_query(QUERY, {c: v.dtype for c, v in table.items()})

    got = f.forward(table)
    want = frame.query(QUERY)
    assert all(np.array_equal(got[c].cpu().numpy(), want[c].to_numpy()) for c in host), "filter_query differs from DataFrame.query"
    kept = len(want)

    inputs = [obs.float_column(table[name], dev) for name in program.inputs]
    code = [(native.EXPR_OPS[op], a, b) for op, a, b in program.code]
    words = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
    counts = torch.empty((n + native.EXPR_CHUNK_ROWS - 1) // native.EXPR_CHUNK_ROWS, dtype=torch.int64, device=dev)
    native.obs_row_expr(code, inputs, program.consts, [], n, keep_words=words, chunk_counts=counts)
    offsets = torch.cumsum(counts, 0) - counts
    positions = torch.empty(kept, dtype=torch.int64, device=dev)
    variants = {
        "filter_query_forward": lambda: f.forward(table),
        "query_rows": lambda: obs.query_rows(table, program, dev=dev),
        "row_expr_launch": lambda: native.obs_row_expr(code, inputs, program.consts, [], n, keep_words=words, chunk_counts=counts),
        "keep_positions_launch": lambda: native.obs_keep_positions(words, offsets, n, positions),
        "torch_isin_nonzero": lambda: torch.nonzero(torch.isin(table["varno"], torch.tensor([1, 2, 3, 4, 7, 59], device=dev))
                                                    & torch.isin(table["pressure"], torch.tensor([85000.0, 92500.0, 100000.0], device=dev))),
    }
    device = interleaved(variants, args.rounds)
    pandas = host_ms(lambda: frame.query(QUERY))
    result = {
        "rows": n, "kept": kept, "query": QUERY, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev),
        "program": {"instructions": len(program.code), "inputs": len(program.inputs), "consts": len(program.consts), "depth": program.depth},
        "bytes_per_row": {"row_expr_launch_read": 8 * len(program.inputs), "row_expr_launch_written": 1 / 8 + 8 / native.EXPR_CHUNK_ROWS,
                          "keep_positions_read": 1 / 8 + 8 / native.EXPR_CHUNK_ROWS, "keep_positions_written_per_kept_row": 8,
                          "varno_to_float64_read_and_written": 16, "gather_per_kept_row_and_column": 16},
        "device_ms": {name: {"median": m, "min": lo, "max": hi} for name, (m, lo, hi) in device.items()},
        "pandas_query_host": pandas, "host_cpus": os.cpu_count(),
    }
    line = json.dumps(result, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
