#!/usr/bin/env python3
"""The tabular QC filters on one MI355X at --rows resident rows: every filter once as its own ``forward`` over a table of device tensors
(the row-program kernel route: compile, upload the scalars, launch, narrow, and for the row-dropping ones ``nonzero`` and the gather),
once as the same statement composed of torch operations on the device, and once as the reference's statement in pandas on this host's
CPU.  Beside them a plain 16-byte-per-row copy of one float64 column, the floor of anything that reads and writes a column once.

    python tools/obs_qc_bench.py --out profiles/obs_qc_bench.json [--rows 10000000]

Device variants are timed with device events, one call at a time, INTERLEAVED over --rounds rounds after a warm-up of every one of them,
so that a stall of the shared host falls on all alike; the median is reported with the smallest and largest reading.  An event pair
around a whole ``forward`` also counts the host's share (the compiler, the allocations, one synchronising reduction where an integer
column decides its dtype).  pandas: one warm-up call, the median of three.  The torch compositions are checked against the filters'
results, bit for bit, before anything is timed."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as graft  # noqa: E402

NAN = float("nan")
DAY_NS = 86400 * 10**9


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
    return {name: (float(np.median(ms)), float(min(ms)), float(max(ms)))
            for name, ms in ((name, [a.elapsed_time(b) for a, b in pairs]) for name, pairs in events.items())}


def host_ms(fn, repeats: int = 3) -> dict:
    fn()
    readings = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        readings.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(readings)), "ms_min": min(readings), "ms_max": max(readings), "repeats": repeats}


def build_table(n: int) -> dict:
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n) * 3.0
    a[rng.random(n) < 0.05] = np.nan
    a[rng.random(n) < 0.01] = np.inf
    b = (rng.standard_normal(n) * 3.0).astype(np.float32)
    b[rng.random(n) < 0.05] = np.nan
    t = 273.15 + rng.standard_normal(n) * 5.0
    td = t - rng.standard_normal(n) * 2.0
    q = rng.random(n) * 0.02
    date = np.datetime64("2024-12-28", "ns").view(np.int64) + rng.integers(0, 12 * 86400, n) * 10**9
    lat, lon = rng.uniform(-90, 90, n), rng.uniform(-180, 180, n)
    lat[rng.random(n) < 0.01] = 2e10
    return {"a": a, "b": b, "2t": t, "2d": td, "2q": q, "latitude": lat, "longitude": lon, "date": date}


def cases(table: dict, dev) -> list:
    """``(name, filter name, config, bytes per row, torch composition, pandas statement)``: the compositions return what the filter
    changes — ``{column: tensor}`` or the kept positions."""
    nan = torch.tensor(NAN, dtype=torch.float64, device=dev)
    nan32 = torch.tensor(NAN, dtype=torch.float32, device=dev)
    f32 = lambda v: float(np.float32(v))  # noqa: E731  the number as the float32 compare sees it

    def where(cond, x):
        return torch.where(cond, nan32 if x.dtype == torch.float32 else nan, x)

    d0, d1, d2, d3 = (int((np.datetime64(s) - np.datetime64("1970-01-01")) // np.timedelta64(1, "D")) for s in
                      ("2025-01-01", "2025-01-02", "2025-01-05", "2025-01-05"))
    import pandas as pd

    ts = lambda s: pd.to_datetime(s, format="%Y%m%d")  # noqa: E731

    def t_exclude(T):
        day = torch.div(T["date"], DAY_NS, rounding_mode="floor")
        return {"a": where(((day >= d0) & (day < d1 + 1)) | ((day >= d2) & (day < d3 + 1)), T["a"])}

    def p_exclude(df):
        x = df["a"]
        for s, e in (("20250101", "20250102"), ("20250105", "20250105")):
            x = x.mask((df["date"] >= ts(s)) & (df["date"] < ts(e) + pd.Timedelta(days=1)))
        return x

    extreme = ["a", "b", "latitude", "longitude"]
    return [
        ("mask_tabular", "mask_tabular", {"a": {"value": 2.5, "operator": ">="}, "b": {"value": 0.1, "operator": ">"}}, 16 + 8,
         lambda T: {"a": where(T["a"] >= 2.5, T["a"]), "b": where(T["b"] > f32(0.1), T["b"])},
         lambda df: (df["a"].mask(df["a"] >= 2.5), df["b"].mask(df["b"] > 0.1))),
        ("mask_outside_range", "mask_outside_range", {"a": [-3.0, 2.5], "b": [-3.0, 0.1]}, 16 + 8,
         lambda T: {"a": where((T["a"] < -3.0) | (T["a"] > 2.5), T["a"]), "b": where((T["b"] < -3.0) | (T["b"] > f32(0.1)), T["b"])},
         lambda df: (df["a"].mask((df["a"] < -3.0) | (df["a"] > 2.5)), df["b"].mask((df["b"] < -3.0) | (df["b"] > 0.1)))),
        ("mask_infs", "mask_infs", {"columns": ["a", "b"]}, 16 + 8,
         lambda T: {c: where(torch.isinf(T[c]), T[c]) for c in ("a", "b")},
         lambda df: [df[c].mask(df[c] == np.inf).mask(df[c] == -np.inf) for c in ("a", "b")]),
        ("mask_dewpoint_temperature", "mask_dewpoint_temperature", {"mask_specific_humidity": True}, 8 + 16 + 16,
         lambda T: {"2d": where(T["2t"] < T["2d"], T["2d"]), "2q": where(T["2t"] < T["2d"], T["2q"])},
         lambda df: (df["2d"].mask(df["2t"] < df["2d"]), df["2q"].mask(df["2t"] < df["2d"]))),
        ("exclude_dates", "exclude_dates", {"a": [[20250101, 20250102], [20250105, 20250105]]}, 8 + 8 + 16 + 16, t_exclude, p_exclude),
        ("remove_extreme_values mask", "remove_extreme_values", {"columns": ["a", "b"], "method": "mask", "threshold": 1e10}, 16 * 3 + 8,
         lambda T: {c: where(T[c].abs() > (f32(1e10) if c == "b" else 1e10), T[c]) for c in extreme},
         lambda df: df[extreme].mask(df[extreme].abs() > 1e10)),
        ("remove_extreme_values drop", "remove_extreme_values", {"columns": ["a", "b"], "method": "drop", "threshold": 1e10}, None,
         lambda T: torch.nonzero(~((T["a"].abs() > 1e10) | (T["b"].abs() > f32(1e10)) | (T["latitude"].abs() > 1e10) | (T["longitude"].abs() > 1e10))).reshape(-1),
         lambda df: df[~(df[extreme].abs() > 1e10).any(axis=1)]),
        ("clip_tabular", "clip_tabular", {"a": [-1.0, 1.0], "b": [0.1, 2.5]}, 16 + 8,
         lambda T: {"a": torch.where(T["a"] > 1.0, 1.0, torch.where(T["a"] < -1.0, -1.0, T["a"])),
                    "b": torch.where(T["b"] > 2.5, 2.5, torch.where(T["b"] < f32(0.1), f32(0.1), T["b"])).to(torch.float32)},
         lambda df: (df["a"].clip(-1.0, 1.0), df["b"].clip(0.1, 2.5))),
        ("impute_nans_tabular", "impute_nans_tabular", {"value": {"a": 0.0, "b": 0.5}}, 16 + 8,
         lambda T: {"a": torch.where(T["a"] != T["a"], 0.0, T["a"]), "b": torch.where(T["b"] != T["b"], 0.5, T["b"]).to(torch.float32)},
         lambda df: df[["a", "b"]].fillna({"a": 0.0, "b": 0.5})),
        ("drop_nans_tabular", "drop_nans_tabular", {"how": "any", "columns": ["a", "b"]}, None,
         lambda T: torch.nonzero(~(torch.isnan(T["a"]) | torch.isnan(T["b"]))).reshape(-1),
         lambda df: df.dropna(how="any", subset=["a", "b"])),
    ]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="recorded in the result: the commit the library was built from")
    ap.add_argument("--no-pandas", action="store_true")
    args = ap.parse_args()
    graft.load_package()
    from anemoi_transform_amd import native, obs
    from anemoi_transform_amd.filters import create_filter_by_name
    from anemoi_transform_amd.tables import Table

    if not torch.cuda.is_available():
        raise SystemExit("obs_qc_bench needs an MI355X: a time taken anywhere else says nothing about it")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.rows
    host = build_table(n)
    T = {c: torch.from_numpy(v).to(dev) for c, v in host.items()}
    scratch = torch.empty(n, dtype=torch.float64, device=dev)
    variants = {"torch copy_ (16 bytes per row)": lambda: scratch.copy_(T["2t"])}
    res = {"rows": n, "rounds": args.rounds, "commit": args.commit, "device": torch.cuda.get_device_name(0), "filters": {}}
    listed = cases(T, dev)
    for name, filter_name, config, per_row, composed, _ in listed:
        f = create_filter_by_name(filter_name, **config)
        got, want = f.forward(T), composed(T)
        if isinstance(want, dict):  # the composition is the filter's statement, to the bit
            same = all(got[c].dtype == w.dtype and np.array_equal(got[c].cpu().numpy().view(np.uint8), w.cpu().numpy().view(np.uint8)) for c, w in want.items())
        else:
            same = got["a"].numel() == want.numel() and torch.equal(got["a"].view(torch.int64), T["a"][want].view(torch.int64))
        del got, want
        res["filters"][name] = {"config": config, "composition_equals_filter": bool(same), "bytes_per_row_by_count": per_row}
        variants[f"{name}: filter"] = (lambda f=f: f.forward(T))
        if per_row is None:  # the row-dropping filters: the composition takes its rows with the same gather
            variants[f"{name}: torch"] = (lambda composed=composed: Table(T).take(composed(T)))
        else:
            variants[f"{name}: torch"] = (lambda composed=composed: composed(T))
    # the kernel alone, without the host's share of a forward: one launch of the mask_tabular program over prebuilt arguments
    program = obs.compile_mask_values({"a": (">=", 2.5)}, {"a": np.dtype("f8")})
    scalars = torch.tensor(program.scalars, dtype=torch.float64, device=dev)
    ops = [(native.ROW_OPS[s.op], s.src, scalars[s.scalar:s.scalar + 1] if s.op == "scalar" else (T["a"] if s.read else None),
            scratch if s.store else None) for s in program.launches[0].slots]
    variants["one launch: a >= 2.5 masked (16 bytes per row)"] = lambda: native.obs_column_ops(ops, n)
    torch.cuda.synchronize()
    for name, (ms, lo, hi) in interleaved(variants, args.rounds).items():
        record = {"ms": ms, "ms_min": lo, "ms_max": hi}
        if "16 bytes per row" in name:
            record["bytes_per_s"] = 16 * n / (ms * 1e-3)
            res.setdefault("streams", {})[name] = record
        else:
            label, kind = name.rsplit(": ", 1)
            per_row = res["filters"][label]["bytes_per_row_by_count"]
            if per_row and kind == "filter":
                record["bytes_per_s_by_count"] = per_row * n / (ms * 1e-3)
            res["filters"][label][kind] = record
        print(f"{name:60s} {ms:9.4f} ms  [{lo:.4f}, {hi:.4f}]", flush=True)
    if not args.no_pandas:
        import pandas as pd

        df = pd.DataFrame({**{c: v for c, v in host.items() if c != "date"}, "date": host["date"].view("datetime64[ns]")})
        for name, _, _, _, _, statement in listed:
            res["filters"][name]["pandas"] = host_ms(lambda statement=statement: statement(df))
            print(f"pandas {name:53s} {res['filters'][name]['pandas']['ms']:9.1f} ms", flush=True)
        res["pandas_threads"] = 1
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
