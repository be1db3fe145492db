#!/usr/bin/env python3
"""Interleaved A/B timing of libatx builds on the bench workload (one process, one GPU).

    bash tools/build_variant.sh parent --rev HEAD~1
    python tools/ab_bench.py --libs parent=anemoi-transform_amd/lib/variants/libatx_parent.so new=anemoi-transform_amd/lib/libatx.so \
        --tiles 0 16 24 --rounds 7 --cases k4f32 k1f32 k4f64

(The gather's compile-time knobs are frozen, HISTORY.md: variants are builds of other commits.)

A case is k<k>f<bits>[e][@shard|@fields]: "e" adds the 2-stage epilogue of config 5, "@shard" times the slowest of the 8
traffic-balanced target shards (tools/shard_efficiency.py's shapes) instead of all targets, "@fields" the field-major stack.

Every (library, tile) pair is timed in every round, rounds interleaved
(cdna_hip_programming.md §5.4 rule 24); reports median / min ms per launch and the
roofline fraction on algorithmic bytes.  A round holds --reps batches of --inner launches per pair; its figure is the median of
the batches.  Against the FIRST library of --libs (the baseline) every other library of the same tile gets
    spread         (max - min of the baseline's round medians) / the baseline's median: its own round-to-round scatter,
    ratio          baseline median / this median,
    below_every_round   this round median < the baseline's, in every round,
    faster         below_every_round and ratio - 1 > 3 x spread  (a real difference has to stand clear of the scatter),
    slower         1 / ratio - 1 > spread.
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
import bench  # noqa: E402


def verdict(base_rounds, rounds):
    """The A/B rule of the docstring on two lists of round medians."""
    base_med, med = float(np.median(base_rounds)), float(np.median(rounds))
    spread = (max(base_rounds) - min(base_rounds)) / base_med
    ratio = base_med / med
    below = all(r < b for r, b in zip(rounds, base_rounds))
    return {"baseline_spread": spread, "ratio": ratio, "below_every_round": below, "faster": bool(below and ratio - 1.0 > 3.0 * spread),
            "slower": bool(1.0 / ratio - 1.0 > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", required=True, help="name=path pairs; the first is the baseline")
    ap.add_argument("--tiles", nargs="+", type=int, default=[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3, help="batches per round and pair")
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--cases", nargs="+", default=["k4f32"])
    ap.add_argument("--levels", type=int, default=137)
    ap.add_argument("--src-grid", default="o1280")
    ap.add_argument("--tgt-grid", default="0.25")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    graft.load_package()
    from anemoi_transform_amd import native
    from anemoi_transform_amd.gather import GatherPlan
    from anemoi_transform_amd.grids import lookup
    from anemoi_transform_amd.interp import knn_inverse_distance
    from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    libs = {}
    for spec in args.libs:
        name, path = spec.split("=", 1)
        libs[name] = native.open_library(os.path.join(ROOT, path) if not os.path.isabs(path) else path, older_build=True)
    baseline = next(iter(libs))

    src_grid, tgt_grid = lookup(args.src_grid), lookup(args.tgt_grid)
    n_src, n_all = len(src_grid["latitudes"]), len(tgt_grid["latitudes"])
    idx_all, w_all = knn_inverse_distance(src_grid, tgt_grid, k=4)
    stream = torch.cuda.current_stream().cuda_stream
    results = {}
    if args.out and os.path.exists(args.out):
        results = json.load(open(args.out))
    for case in args.cases:
        shape, _, where = case.partition("@")
        assert where in ("", "shard", "fields"), case
        k = int(shape[1])
        f64 = "f64" in shape
        tdt, npdt, isz = (torch.float64, np.float64, 8) if f64 else (torch.float32, np.float32, 4)
        layout = FIELDS if where == "fields" else COLUMNS
        src = bench.synth_stack(src_grid, args.levels, tdt, dev, 0, COLUMNS)
        if layout == FIELDS:
            src = src.to_layout(FIELDS)

        # "...e": with the 2-stage epilogue of config 5 (x * g, then x - 273.15)
        prog = native.level_program([[(native.OP_MUL, 0, 9.80665, 0.0)] * args.levels, [(native.OP_AFFINE, 0, 1.0, -273.15)] * args.levels],
                                    dev) if "e" in shape[2:] else None
        vec_p, host_p = native._program_companions(prog, tdt)

        def tables(lo, hi):
            idx = torch.from_numpy(np.ascontiguousarray(idx_all[lo:hi, :k]).astype(np.int32)).to(dev)
            w = torch.from_numpy(np.ascontiguousarray(w_all[lo:hi]).astype(npdt)).to(dev) if k > 1 else None
            return idx, w, Stack.empty(hi - lo, args.levels, tdt, dev, layout)

        def launch(h, tile, idx, w, out):
            h.atx_set_tuning(tile)
            rc = h.atx_regrid_ell(src.data.data_ptr(), out.data.data_ptr(), idx.data_ptr(), None if w is None else w.data_ptr(),
                                  n_src, out.n_pts, k, args.levels, src.pitch, out.pitch, 1 if f64 else 0, layout, 0,
                                  None if prog is None else prog.data_ptr(), vec_p, host_p, 0 if prog is None else 2, None, stream)
            assert rc == 0, h.atx_last_error()

        def batch_ms(h, tile, idx, w, out, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                launch(h, tile, idx, w, out)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / n

        lo, hi = 0, n_all
        if where == "shard":  # the slowest of the 8 traffic-balanced shards, found with the baseline
            cut = GatherPlan(n_src, n_all, index=idx_all, weights=w_all).bounds(8)
            cost = []
            for r in range(8):
                t = tables(cut[r], cut[r + 1])
                batch_ms(libs[baseline], 0, *t, 3)
                cost.append(batch_ms(libs[baseline], 0, *t, args.inner))
                del t
            r = int(np.argmax(cost))
            lo, hi = int(cut[r]), int(cut[r + 1])
            print(f"{case}: shard {r} of 8, targets [{lo}, {hi}), per-shard ms {np.round(cost, 4).tolist()}", flush=True)
        idx, w, out = tables(lo, hi)
        alg = bench.algorithmic_bytes(args.levels, isz, int(np.unique(idx_all[lo:hi, :k]).size), hi - lo, k)

        tiles = [0] if layout == FIELDS else args.tiles  # (the tuning hook selects among the column kernels only)
        combos = [(name, tile) for name in libs for tile in tiles]
        rounds = {c: [] for c in combos}
        batches = {c: [] for c in combos}
        ref_out = None
        for c in combos:  # warm-up + every variant must produce the same bits
            out.data.fill_(float("nan"))
            launch(libs[c[0]], c[1], idx, w, out)
            torch.cuda.synchronize()
            if ref_out is None:
                ref_out = out.data.clone()
            else:
                same = torch.equal(out.data.view(torch.int32 if not f64 else torch.int64), ref_out.view(torch.int32 if not f64 else torch.int64))
                assert same, f"variant {c} differs from {combos[0]}"
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for c in combos:
                ms = [batch_ms(libs[c[0]], c[1], idx, w, out, args.inner) for _ in range(args.reps)]
                batches[c] += ms
                rounds[c].append(float(np.median(ms)))
        for c in combos:
            med, mn = float(np.median(batches[c])), float(np.min(batches[c]))
            rec = {"median_ms": med, "min_ms": mn, "frac_median": alg / (med * 1e-3) / 8e12, "frac_min": alg / (mn * 1e-3) / 8e12,
                   "round_medians_ms": rounds[c], "spread": (max(rounds[c]) - min(rounds[c])) / float(np.median(rounds[c]))}
            note = ""
            if c[0] != baseline:
                rec["vs_" + baseline] = v = verdict(rounds[(baseline, c[1])], rounds[c])
                note = f"  ratio {v['ratio']:.4f} (3 x spread {3 * v['baseline_spread']:.4f})" + ("  FASTER" if v["faster"] else "  slower" if v["slower"] else "")
            results[f"{case}/{c[0]}/tile{c[1]}"] = rec
            print(f"{case:14s} {c[0]:10s} tile={c[1]:3d}  median {med:.4f} ms  min {mn:.4f} ms  frac {alg / (med * 1e-3) / 8e12:.4f}  spread {rec['spread']:.4f}{note}",
                  flush=True)
        del src, out, idx, w
        torch.cuda.empty_cache()
        if args.out:  # after every case: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
