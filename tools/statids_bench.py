#!/usr/bin/env python3
"""atx_text_encode_statids and the encode_statids filter on one MI355X, beside the reference's statement in pandas on this host's CPU.

    python tools/statids_bench.py --out profiles/statids_bench.json [--rows 10000000] [--cpu-rows 200000]

(a) the kernel alone on a resident byte matrix at widths 8 and 16: identifiers that are all base-36 numbers, all MD5 rows, and a seeded
    mix of 70 % numbers, 25 % MD5 rows and 5 % rows the kernel leaves undecided — each beside a plain torch copy of the same bytes per
    row (width read, 9 written: width + 9), which is the byte bound of the launch;
(b) ``EncodeStatids.forward`` of the mix from a host object column and from a ``U`` array, split into pack (``tables.text_matrix``),
    upload, launch and the host-decided rows;
(c) the reference's statement through ``Series.apply`` on --cpu-rows rows, one process, scaled to --rows.

The kernel variants are timed with device events, one call at a time, INTERLEAVED over --rounds rounds after a warm-up of every one, so
that a stall of the shared host falls on all alike; the median is reported with the smallest and largest reading.  Host steps: the
median of three wall-clock readings.
"""

from __future__ import annotations

import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import __graft_entry__ as graft  # noqa: E402
from column_ops_bench import interleaved  # noqa: E402


@functools.lru_cache(maxsize=None)
def identifiers(n: int, kind: str, seed: int = 20261020) -> np.ndarray:
    """A ``U`` array of n identifiers of at most 7 characters: ``numbers`` (WMO-style digits and ICAO-style letters), ``md5`` (a ``-``
    inside) or ``mix``: 70 % numbers, 25 % md5, 5 % non-ASCII."""
    rng = np.random.default_rng(seed)
    number = np.char.zfill(rng.integers(1000, 99999, size=n).astype("U5"), 5)
    dashed = np.char.add(np.char.add(rng.integers(10, 999, size=n).astype("U3"), "-"), rng.integers(0, 999, size=n).astype("U3"))
    if kind == "numbers":
        return number
    if kind == "md5":
        return dashed
    pick = rng.integers(0, 100, size=n)
    return np.where(pick < 70, number, np.where(pick < 95, dashed, np.char.add("Ø", number)))


def wall(fn, repeats: int = 3) -> tuple[float, object]:
    times, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cpu-rows", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    graft.load_package()
    from anemoi_transform_amd import native_text, obs, tables
    from anemoi_transform_amd.filters import create_filter_by_name

    dev = torch.device("cuda", 0)
    n = args.rows
    record: dict = {"rows": n, "device": torch.cuda.get_device_name(0)}

    # (a) the kernel alone
    variants, keep = {}, []
    for width in (8, 16):
        for kind in ("numbers", "md5", "mix"):
            text, w = tables.text_matrix(identifiers(n, kind))
            matrix = np.zeros((n, width), dtype=np.uint8)
            matrix[:, :w] = text[:, :w]
            t = torch.from_numpy(matrix).to(dev)
            code, flag = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
            keep.append((t, code, flag))
            variants[f"kernel width {width} {kind}"] = lambda t=t, code=code, flag=flag: native_text.encode_statids(t, code, flag)
        src = torch.empty(n * (width + 9) // 2, dtype=torch.uint8, device=dev)  # as many bytes read, as many written, as the launch moves
        dst = torch.empty_like(src)
        keep.append((src, dst))
        variants[f"copy of width + 9 = {width + 9} bytes per row"] = lambda src=src, dst=dst: dst.copy_(src)
    timed = interleaved(variants, args.rounds)
    record["kernel"] = {}
    for name, (median, low, high) in timed.items():
        width = 8 if " 8 " in name or "= 17" in name else 16
        record["kernel"][name] = {"ms": median, "min_ms": low, "max_ms": high, "GBs_on_width_plus_9": n * (width + 9) / median / 1e6,
                                  "rows_per_s": n / median * 1e3}
        print(f"{name:45s} {median:8.3f} ms  [{low:.3f}, {high:.3f}]  {n * (width + 9) / median / 1e6:8.1f} GB/s", flush=True)
    for width in (8, 16):
        copy = record["kernel"][f"copy of width + 9 = {width + 9} bytes per row"]["ms"]
        for kind in ("numbers", "md5", "mix"):
            entry = record["kernel"][f"kernel width {width} {kind}"]
            entry["times_the_copy"] = entry["ms"] / copy
            entry["nearer_bound"] = "bytes" if entry["ms"] < 2.0 * copy else "VALU"
    del keep, variants

    # (b) forward, from a host column
    record["forward"] = {}
    for source in ("object", "U"):
        ids = identifiers(n, "mix")
        column = ids.astype(object) if source == "object" else ids
        pack_ms, (text, width) = wall(lambda: tables.text_matrix(column))
        upload_ms, t = wall(lambda: torch.from_numpy(text).to(dev))
        code, flag = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        launch_ms, _ = wall(lambda: native_text.encode_statids(t[:, :width], code, flag))
        f = create_filter_by_name("encode_statids")
        forward_ms, _ = wall(lambda: f({"statid": column}))
        rows = torch.nonzero(flag).reshape(-1).cpu().tolist()
        host_ms, _ = wall(lambda: [obs.statid_to_int(ids[i]) for i in rows])
        record["forward"][source] = {"forward_ms": forward_ms, "pack_ms": pack_ms, "upload_ms": upload_ms, "launch_ms": launch_ms,
                                     "host_rows": f.last_host_rows, "host_rows_ms": host_ms, "pitch": int(text.shape[1]), "width": int(width)}
        print(source, record["forward"][source], flush=True)

    # (c) the reference's statement in pandas, one process
    import pandas as pd

    series = pd.Series(identifiers(args.cpu_rows, "mix").astype(object))
    series.apply(obs.statid_to_int)
    cpu_ms, _ = wall(lambda: series.apply(obs.statid_to_int))
    record["pandas_apply"] = {"rows": args.cpu_rows, "ms": cpu_ms, "scaled_to_rows_s": cpu_ms * n / args.cpu_rows / 1e3, "pandas": pd.__version__}
    print(record["pandas_apply"], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
