#!/usr/bin/env python3
"""atx_obs_column_ops on one MI355X: the time of each of the ten functions alone over --rows float64 rows (8 bytes read, 8 written per
row) beside a plain 16-byte-per-row stream of the same rows (torch copy_ and libatx's stream_copy, as tools/hbm_ceiling.py measures
them); `safe_log + sin_deg + cos_deg + exp` from two source columns as ONE launch against the same four as four launches; and numpy on
this host's CPU for the same statements.

    python tools/column_ops_bench.py --out profiles/column_ops_bench.json [--rows 10000000] [--ulps profiles/column_ops_ulps.json]

Every variant is timed with device events, one call at a time, the variants INTERLEAVED over --rounds rounds after a warm-up of every
one of them, so that a stall of the shared host falls on all alike; the median is reported with the smallest and largest reading.
An event pair around one call of 25 - 80 microseconds also counts what the host does before the launch when the queue has drained;
--only FUNCTION under a kernel trace gives the kernel's own duration.  numpy: one warm-up call, the median of three.
--ulps: also the worst distance of every function from exact arithmetic on the generators of tests/column_ops_restatement.py."""

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

FUSED = [("lnsp", "sp", "safe_log"), ("sin_dd", "dd", "sin_deg"), ("cos_dd", "dd", "cos_deg"), ("sp_again", "lnsp", "exp")]


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


def measure_ulps(obs) -> dict:
    import column_ops_restatement as R

    out = {}
    for function in R.FUNCTIONS:
        x = R.cases(function)
        got = obs.column_ops({"x": torch.from_numpy(x).cuda()}, [("y", "x", function)])["y"].cpu().numpy()
        with np.errstate(all="ignore"):
            want = R.NUMPY[function](x)
        if function in R.BIT_EQUAL:
            out[function] = {"cases": int(x.size), "rows_unlike_numpy": int((~(np.isnan(got) & np.isnan(want)) & (got.view(np.int64) != want.view(np.int64))).sum())}
            continue
        exact = R.exact_cases(function)
        err, err_numpy = R.X.ulp_errors(got, exact, np.float64), R.X.ulp_errors(want, exact, np.float64)
        far = np.abs(R.argument(function, x)) >= 1.0e5
        record = {"cases": int(x.size), "kernel_ulps": float(err.max()), "numpy_ulps": float(err_numpy.max()), "budget_ulps": 1.0,
                  "kernel_worst_at": float(x[int(np.argmax(err))])}
        if function in ("sin", "sin_deg", "cos", "cos_deg"):
            record.update(kernel_ulps=float(err[~far].max()), numpy_ulps=float(err_numpy[~far].max()), kernel_ulps_beyond_1e5=float(err[far].max()),
                          numpy_ulps_beyond_1e5=float(err_numpy[far].max()), budget_ulps_beyond_1e5=2.0)
        out[function] = record
        print(f"{function:9s} {record}", flush=True)
    return out


def summarise_trace(directory: str) -> dict:
    """{kernel name: {calls, median / min / max microseconds}} of every *kernel_trace.csv under `directory` — what a run of
    `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/column_ops_bench.py --only FUNCTION` left there."""
    import csv
    import glob

    spans: dict = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                spans.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {name: {"calls": len(us), "us_median": float(np.median(us)), "us_min": min(us), "us_max": max(us)} for name, us in spans.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ulps", default=None, help="also measure every function against exact arithmetic and write the record here")
    ap.add_argument("--only", default=None, help="time this one function (and the two copies) and stop: under a kernel trace the kernel's own "
                    "duration, without the host's share of an event pair around a 50 microsecond call")
    ap.add_argument("--commit", default=None, help="recorded in the result: the commit the library was built from")
    ap.add_argument("--summarise-trace", default=None, metavar="DIR", help="no GPU work: kernel durations from the kernel-trace csv files "
                    "under DIR, written to --out")
    args = ap.parse_args()
    if args.summarise_trace:
        kernels = summarise_trace(args.summarise_trace)
        for name, rec in sorted(kernels.items(), key=lambda kv: -kv[1]["calls"])[:8]:
            print(f"{rec['calls']:6d} calls  {rec['us_median']:8.2f} us  [{rec['us_min']:.2f}, {rec['us_max']:.2f}]  {name[:100]}")
        if args.out:
            with open(args.out, "w") as f:
                json.dump({"only": args.only, "kernels": kernels}, f, indent=1)
        return
    graft.load_package()
    import column_ops_restatement as R
    from anemoi_transform_amd import native, obs

    if not torch.cuda.is_available():
        raise SystemExit("column_ops_bench needs an MI355X: a time taken anywhere else says nothing about it")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.rows
    rng = np.random.default_rng(n)
    host = {"sp": rng.uniform(5.0e4, 1.05e5, n), "dd": rng.uniform(0.0, 360.0, n), "x": rng.uniform(-10.0, 10.0, n)}
    source = {"log": "sp", "log1p": "sp", "safe_log": "sp", "sqrt": "sp", "exp": "x", "abs": "x", "sin": "x", "sin_deg": "dd", "cos": "x", "cos_deg": "dd"}
    cols = {name: torch.from_numpy(col).to(dev) for name, col in host.items()}
    outs = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(4)]
    code = native.COLUMN_OPS

    variants = {"torch copy_ (16 bytes per row)": lambda: outs[0].copy_(cols["x"]),
                "libatx stream_copy (16 bytes per row)": lambda: native.stream_copy(cols["x"], outs[0])}
    for function in R.FUNCTIONS:
        variants[function] = (lambda f=function: native.obs_column_ops([(code[f], -1, cols[source[f]], outs[0])], n))
    # the four of FUSED: one launch (exp takes safe_log's result from a register) against four (exp reads it back)
    variants["four in one launch"] = lambda: native.obs_column_ops(
        [(code["safe_log"], -1, cols["sp"], outs[0]), (code["sin_deg"], -1, cols["dd"], outs[1]), (code["cos_deg"], -1, cols["dd"], outs[2]),
         (code["exp"], 0, None, outs[3])], n)

    def four_launches():
        native.obs_column_ops([(code["safe_log"], -1, cols["sp"], outs[0])], n)
        native.obs_column_ops([(code["sin_deg"], -1, cols["dd"], outs[1])], n)
        native.obs_column_ops([(code["cos_deg"], -1, cols["dd"], outs[2])], n)
        native.obs_column_ops([(code["exp"], -1, outs[0], outs[3])], n)

    variants["four in four launches"] = four_launches
    if args.only:  # for a kernel-trace run of its own: every dispatch of obs_column_ops_kernel in the trace is this one function
        variants = {name: fn for name, fn in variants.items() if name == args.only or "16 bytes per row" in name}
        for name, (ms, lo, hi) in interleaved(variants, args.rounds).items():
            print(f"{name:40s} {ms:8.4f} ms  [{lo:.4f}, {hi:.4f}]", flush=True)
        return
    times = interleaved(variants, args.rounds)
    traffic = {name: 16 * n for name in variants}
    traffic["four in one launch"] = (2 + 4) * 8 * n  # sp and dd read once, four columns written
    traffic["four in four launches"] = (4 + 4) * 8 * n  # a read and a write each
    res = {"rows": n, "rounds": args.rounds, "commit": args.commit, "device": torch.cuda.get_device_name(0), "variants": {}}
    for name, (ms, lo, hi) in times.items():
        res["variants"][name] = {"ms": ms, "ms_min": lo, "ms_max": hi, "bytes": traffic[name], "bytes_per_s": traffic[name] / (ms * 1e-3),
                                 "rows_per_s": n / (ms * 1e-3)}
        print(f"{name:40s} {ms:8.4f} ms  [{lo:.4f}, {hi:.4f}]  {traffic[name] / (ms * 1e-3) / 1e12:6.3f} TB/s", flush=True)
    # the fused launch computes what the four launches compute
    one = obs.column_ops(cols, FUSED)
    table = dict(cols)
    for op in FUSED:
        table.update(obs.column_ops(table, [op]))
    res["fused_equals_one_by_one"] = all(torch.equal(one[t].view(torch.int64), table[t].view(torch.int64)) for t in one)
    # numpy on this host, one process
    res["numpy"] = {}
    def host_ms(fn, repeats=3):
        """Median of `repeats` wall-clock readings after one warm-up call (the first call pays for the pages of its output)."""
        fn()
        readings = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            readings.append((time.perf_counter() - t0) * 1e3)
        return {"ms": float(np.median(readings)), "ms_min": min(readings), "ms_max": max(readings), "repeats": repeats}

    with np.errstate(all="ignore"):
        for function in R.FUNCTIONS:
            res["numpy"][function] = host_ms(lambda f=function: R.NUMPY[f](host[source[f]]))
        res["numpy"]["four"] = host_ms(lambda: R.interpret(FUSED, host))
    for name, rec in res["numpy"].items():
        print(f"numpy {name:34s} {rec['ms']:8.1f} ms", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.ulps:
        with open(args.ulps, "w") as f:
            json.dump({"commit": args.commit, "device": torch.cuda.get_device_name(0), "functions": measure_ulps(obs)}, f, indent=1)


if __name__ == "__main__":
    main()
