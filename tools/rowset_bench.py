#!/usr/bin/env python3
"""sort_by and drop_duplicates on one MI355X over a table of --rows rows resident in HBM: eight float64 value columns, `date` (int64
nanoseconds, almost all distinct) and an int64 `station` key with about four rows per key; a quarter of the rows repeat the (date,
station) of another row.

    python tools/rowset_bench.py --out profiles/rowset_bench.json [--rows 10000000]

`sort_by(date)` and `drop_duplicates(date, station)` are each split into their three parts — the int64 order keys
(atx_obs_order_key), the stable sort(s) (torch.sort, with atx_obs_mark_first and the compaction for the duplicates) and the gather of
all ten columns (atx_obs_take_rows, one launch) — and timed whole, filter in to dict out.  Beside the fused gather runs
torch.index_select per column on the same tensors and the same row list, for both shapes of list: the random permutation of the
sort and the ascending rows of the duplicates.  The reference's statements (DataFrame.sort_values(kind="stable"),
DataFrame.drop_duplicates) run in pandas on this host's CPU, one process, and the rows they return are compared with the device's.

Every device variant is timed with device events, one call at a time, the variants INTERLEAVED over --rounds rounds after a warm-up
of every one of them, so that a stall of the shared host falls on all alike; the median is reported with the smallest and largest
reading.  pandas: one warm-up call, the median of three."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import __graft_entry__ as graft  # noqa: E402

VALUES = [f"obsvalue_{k}" for k in range(8)]


def interleaved(variants: dict, rounds: int, warm: int = 3) -> dict:
    """{name: (median, min, max) ms} of one call of every variant, the variants taking turns."""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    events = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events[name].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for name, pairs in events.items():
        ms = [a.elapsed_time(b) for a, b in pairs]
        out[name] = (float(np.median(ms)), float(min(ms)), float(max(ms)))
    return out


def build_table(n: int) -> dict:
    """Three quarters of the rows have a date of their own within 30 days and a station out of n / 4; the last quarter copies date and
    station of one of those; one permutation shuffles the rows."""
    rng = np.random.default_rng(n)
    own = n - n // 4
    date = np.int64(1_700_000_000) * 10**9 + rng.integers(0, 30 * 86400 * 10**9, own)
    station = rng.integers(0, max(n // 4, 1), own)
    again = rng.integers(0, own, n - own)
    shuffle = rng.permutation(n)
    table = {"date": np.concatenate([date, date[again]])[shuffle], "station": np.concatenate([station, station[again]])[shuffle]}
    for name in VALUES:
        table[name] = rng.normal(280.0, 30.0, n)
    return table


def host_ms(fn, repeats: int = 3) -> dict:
    """Median of `repeats` wall-clock readings after one warm-up call."""
    fn()
    readings = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        readings.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(readings)), "ms_min": min(readings), "ms_max": max(readings), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="recorded in the result: the commit the library was built from")
    ap.add_argument("--no-pandas", action="store_true", help="skip the CPU statements (and the comparison of the rows with them)")
    args = ap.parse_args()
    graft.load_package()
    from anemoi_transform_amd import obs
    from anemoi_transform_amd.filters import create_filter_by_name

    if not torch.cuda.is_available():
        raise SystemExit("rowset_bench needs an MI355X: a time taken anywhere else says nothing about it")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.rows
    host = build_table(n)
    table = {name: torch.from_numpy(col).to(dev) for name, col in host.items()}
    columns = list(table.values())
    sort_by = create_filter_by_name("sort_by", columns=["date"])
    dedup = create_filter_by_name("drop_duplicates", columns=["date", "station"])

    # the parts, on inputs computed once
    date_key = obs.order_keys(table["date"], datetime=True)
    station_key = obs.order_keys(table["station"])
    perm = torch.sort(date_key, stable=True).indices
    pair_order = obs._sort_keys([date_key, station_key])
    kept = obs.first_rows([table["date"], table["station"]], datetimes=[True, False])
    n_kept = kept.numel()

    def mark_and_compact():
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        obs.native.obs_mark_first([date_key, station_key], pair_order, keep)
        return torch.nonzero(keep).reshape(-1)

    variants = {
        "sort_by: keys (atx_obs_order_key, 1 column)": lambda: obs.order_keys(table["date"], datetime=True),
        "sort_by: sort (torch.sort stable, int64)": lambda: torch.sort(date_key, stable=True),
        "sort_by: take, fused (atx_obs_take_rows, 10 columns, random permutation)": lambda: obs._take(columns, perm, check=False),
        "sort_by: take, torch.index_select per column (random permutation)": lambda: [torch.index_select(c, 0, perm) for c in columns],
        "sort_by: whole filter": lambda: sort_by(table),
        "drop_duplicates: keys (atx_obs_order_key, 2 columns)": lambda: (obs.order_keys(table["date"], datetime=True), obs.order_keys(table["station"])),
        "drop_duplicates: sort (2 stable sorts, 2 one-column takes)": lambda: obs._sort_keys([date_key, station_key]),
        "drop_duplicates: mark (atx_obs_mark_first) and compact (torch.nonzero)": mark_and_compact,
        "drop_duplicates: take, fused (atx_obs_take_rows, 10 columns, ascending rows)": lambda: obs._take(columns, kept, check=False),
        "drop_duplicates: take, torch.index_select per column (ascending rows)": lambda: [torch.index_select(c, 0, kept) for c in columns],
        "drop_duplicates: whole filter": lambda: dedup(table),
    }
    times = interleaved(variants, args.rounds)
    row_bytes = sum(c.element_size() for c in columns)
    res = {"rows": n, "rows_kept_by_drop_duplicates": n_kept, "columns": {name: str(c.dtype) for name, c in table.items()}, "rounds": args.rounds,
           "commit": args.commit, "device": torch.cuda.get_device_name(0), "variants": {}}
    for name, (ms, lo, hi) in times.items():
        rec = {"ms": ms, "ms_min": lo, "ms_max": hi}
        if ": take" in name:  # every column read at the row and written, the row list read once (fused) or once per column
            rows_out = n if name.startswith("sort_by") else n_kept
            rec["bytes"] = rows_out * (2 * row_bytes + 8 * (1 if "fused" in name else len(columns)))
            rec["bytes_per_s"] = rec["bytes"] / (ms * 1e-3)
        res["variants"][name] = rec
        print(f"{name:82s} {ms:9.4f} ms  [{lo:.4f}, {hi:.4f}]", flush=True)

    # the fused gather moves what index_select moves
    fused = obs._take(columns, perm)
    res["fused_take_equals_index_select"] = all(torch.equal(a.view(torch.int64), torch.index_select(c, 0, perm).view(torch.int64))
                                                for a, c in zip(fused, columns))
    if not args.no_pandas:
        import pandas as pd

        frame = pd.DataFrame(host)
        res["pandas"] = {"sort_values(by=date, kind=stable)": host_ms(lambda: frame.sort_values(by=["date"], kind="stable")),
                         "drop_duplicates(subset=(date, station))": host_ms(lambda: frame.drop_duplicates(subset=["date", "station"]))}
        for name, rec in res["pandas"].items():
            print(f"pandas {name:75s} {rec['ms']:9.1f} ms  [{rec['ms_min']:.1f}, {rec['ms_max']:.1f}]", flush=True)
        res["sort_order_equals_pandas"] = bool(np.array_equal(perm.cpu().numpy(), frame.sort_values(by=["date"], kind="stable").index.to_numpy()))
        res["first_rows_equal_pandas"] = bool(np.array_equal(kept.cpu().numpy(), frame.drop_duplicates(subset=["date", "station"]).index.to_numpy()))
        print("rows equal pandas':", res["sort_order_equals_pandas"], res["first_rows_equal_pandas"], flush=True)
    if args.out:
        variants = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in res.pop("variants").items())
        with open(args.out, "w") as f:  # one line per variant
            f.write(json.dumps(res)[:-1] + ', "variants": {\n' + variants + "\n }}\n")


if __name__ == "__main__":
    main()
