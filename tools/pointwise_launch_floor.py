#!/usr/bin/env python3
"""The launch floor of atx_pointwise_stack — or, with --gather, of atx_regrid_ell — two builds of libatx.so side by side in one
process: a 4 KB float32 column stack (256 points x 4 levels, y = a x + b by value; --gather: 1024 targets x 1 level, the pure k = 1
gather), where the call's cost is the host side of one launch.  Per round and build: the wall time of --calls back-to-back calls
ending in a device synchronise, divided by the calls; the builds alternate, --rounds rounds.  The noise is the spread of the FIRST
build's own rounds; the difference of the medians is to be read against it.

    python tools/pointwise_launch_floor.py [--gather] --lib parent=/path/libatx.so this=anemoi-transform_amd/lib/libatx.so --out profiles/x.json
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", nargs="+", required=True, metavar="NAME=PATH")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gather", action="store_true", help="time atx_regrid_ell (k = 1, no weights, a 4 KB one-level stack) instead of atx_pointwise_stack")
    args = ap.parse_args()
    graft.load_package()
    from anemoi_transform_amd import native
    from anemoi_transform_amd.stack import COLUMNS

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    entry = "atx_regrid_ell" if args.gather else "atx_pointwise_stack"

    def open_build(path):  # the one prototype: an older build need not export every symbol of today's header
        handle = ctypes.CDLL(path)
        getattr(handle, entry).restype, getattr(handle, entry).argtypes = native.SIGNATURES[entry]
        return handle

    libs = [(spec.split("=", 1)[0], open_build(spec.split("=", 1)[1])) for spec in args.lib]
    n_pts, n_lev = 256, 4
    x = torch.rand(n_pts, n_lev, dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    prog = native.level_program([[(native.OP_AFFINE, 0, 1.5, -3.0)] * n_lev], dev)
    call_args = (native._ptr(x), native._ptr(y), n_pts, n_lev, n_lev, n_lev, native.F32, COLUMNS, native._ptr(prog),
                 *native._program_companions(prog, torch.float32), 1, None, native._stream())
    case = "atx_pointwise_stack, 256 points x 4 float32 levels (4 KB), one uniform AFFINE stage, out of place"
    if args.gather:
        n_src = n_tgt = 1024
        src = torch.rand(n_src, 1, dtype=torch.float32, device=dev)
        out = torch.empty(n_tgt, 1, dtype=torch.float32, device=dev)
        idx = torch.randperm(n_src, device=dev).to(torch.int32)
        call_args = native._regrid_ell_args(src, out, idx, None, n_src, n_tgt, 1, 1, 1, 1, COLUMNS, None, 0, None, False) + (native._stream(),)
        case = "atx_regrid_ell, k = 1 without weights, 1024 targets x 1 float32 level (4 KB in, 4 KB out), no program"

    def one_round(handle):
        fn = getattr(handle, entry)
        for _ in range(200):
            assert fn(*call_args) == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn(*call_args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.calls * 1e6

    per = {name: [] for name, _ in libs}
    for _ in range(args.rounds):
        for name, handle in libs:
            per[name].append(one_round(handle))
    ref = libs[0][0]
    res = {"case": case, "unit": "us per call (host wall, calls back to back, one synchronise per round)",
           "calls_per_round": args.calls, "rounds": args.rounds, "builds": {}}
    for name, vals in per.items():
        res["builds"][name] = {"median": float(np.median(vals)), "min": float(np.min(vals)), "max": float(np.max(vals)), "rounds": [round(v, 4) for v in vals]}
    res["noise_of_" + ref] = {"spread_min_to_max": res["builds"][ref]["max"] - res["builds"][ref]["min"],
                              "interquartile": float(np.subtract(*np.percentile(per[ref], [75, 25])))}
    for name in per:
        if name != ref:
            res[f"{name}_minus_{ref}_median"] = res["builds"][name]["median"] - res["builds"][ref]["median"]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
