#!/usr/bin/env python3
"""Per-kernel timing of libatx at BASELINE sizes (O1280 stack of 137 levels), with the HBM roofline
fraction of each on its ALGORITHMIC bytes.  One JSON document on stdout / --out.

    python tools/kernel_bench.py --out gpurun_out/kernels.json
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
import bench  # noqa: E402

PEAK = 8e12


def timeit(fn, n=10, warm=2):
    """Median of n per-call HIP-event durations: one call in a few hundred stalls for tens of ms on a shared host (a lone 4.4 ms
    reading among 1.9 ms ones, `profiles/r03_padded_order_probe.log`), which a mean over 10 carries into the table."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in evs]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--levels", type=int, default=137)
    ap.add_argument("--only-vertical", action="store_true", help="only the column kernel (atx_pressure_at_height_stack) rows")
    ap.add_argument("--only-rotate", action="store_true", help="only the vector-frame kernel (atx_rotate_vectors_stack) rows")
    ap.add_argument("--only-obs", action="store_true", help="only the observation-gridding rows (atx_obs_best_per_cell, atx_obs_fill_stack)")
    ap.add_argument("--only-superob", action="store_true", help="only the superob rows (atx_obs_group_mean, atx_obs_group_argmin, the filter end "
                    "to end beside the reference's statement in pandas on this host); --only-obs runs them after its own rows")
    ap.add_argument("--only-rowops", action="store_true", help="only the per-row observation kernels (atx_obs_forcings, atx_obs_view_angles, "
                    "atx_obs_planck_bt) at --rows rows, rows/s beside the reference's numpy statements on this host")
    ap.add_argument("--only-healpix", action="store_true", help="only the HEALPix kernel (atx_healpix_ang2pix) at --rows rows: nest at nside 32 and "
                    "2^29, ring at nside 32, rows/s beside the vectorised numpy restatement on this host (profiles/healpix_bench.json)")
    ap.add_argument("--only-fill-heights", action="store_true", help="only the station-height kernel (atx_obs_fill_heights) at --rows rows, half of "
                    "them to fill, against a 1801 x 3600 float32 orography: rows/s beside cKDTree and fancy indexing on this host, and four rows "
                    "that take the kernel apart (profiles/fill_heights_bench.json)")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--commit", default=None, help="recorded in the --only-rowops / --only-healpix result: the commit the library was built from")
    ap.add_argument("--only-pointwise", action="store_true", help="only the per-point, mask and reduction rows (atx_pointwise.hip, atx_mask.hip, "
                    "atx_reduce.hip), each with a checksum of what it computed on the seeded stack")
    ap.add_argument("--only-regrid", action="store_true", help="only the gather rows (atx_regrid_columns.inc, atx_regrid_fields.inc), each with a "
                    "checksum of what one call writes into a zeroed output stack")
    ap.add_argument("--only-combine", action="store_true", help="only the multi-input, layout and level-selection rows (atx_combine.hip, atx_relayout.hip), "
                    "each with a checksum of what one call writes into zeroed outputs")
    ap.add_argument("--lib", nargs="+", action="extend", default=[], metavar="NAME=PATH", help="with --only-regrid or --only-combine: time these builds of libatx.so side by side in "
                    "one process, alternating, --rounds rounds (the first one is the reference)")
    ap.add_argument("--rounds", type=int, default=8)
    args = ap.parse_args()
    graft.load_package()
    from anemoi_transform_amd import interp, native
    from anemoi_transform_amd.gather import GatherPlan
    from anemoi_transform_amd.grids import lookup
    from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = args.levels
    src_grid, tgt_grid = lookup("o1280"), lookup("0.25")
    n_src, n_tgt = len(src_grid["latitudes"]), len(tgt_grid["latitudes"])
    res = {}

    def record(name, ms, alg_bytes, note=""):
        res[name] = {"ms": ms, "algorithmic_bytes": alg_bytes, "GBs": alg_bytes / ms / 1e6, "frac_of_8TBs": alg_bytes / (ms * 1e-3) / PEAK,
                     "note": note}
        print(f"{name:42s} {ms:9.4f} ms  {alg_bytes / ms / 1e6:9.1f} GB/s  frac {alg_bytes / (ms * 1e-3) / PEAK:.3f}  {note}", flush=True)

    def vertical_rows(tdt, B, tag):
        """The pressure at 2 m and at 1500 m (interpolation between full levels) from L-level t and q stacks, both layouts: one column
        walk per point, two stacks read, one field written — algorithmic bytes 2·L·N·B + 2·N·B (sp in, p out)."""
        eta = torch.cat([torch.zeros(1, dtype=torch.float64), torch.logspace(np.log10(2e-4), 0.0, L, dtype=torch.float64)])
        Bc = torch.clamp((eta - 0.2) / 0.8, 0.0, 1.0) ** 1.5
        Ac, Bc = (101325.0 * (eta - Bc) * 0.9).to(dev), Bc.to(dev)
        sp = (60000.0 + 45000.0 * torch.rand(n_src, device=dev)).to(tdt)
        p = torch.empty(n_src, dtype=tdt, device=dev)
        for layout, lname in ((COLUMNS, "columns"), (FIELDS, "fields")):
            t, q = Stack.empty(n_src, L, tdt, dev, layout, zero=True), Stack.empty(n_src, L, tdt, dev, layout, zero=True)
            tv = t.data[:, :L] if layout == COLUMNS else t.data
            qv = q.data[:, :L] if layout == COLUMNS else q.data
            tv.uniform_(200.0, 300.0)
            qv.copy_(torch.pow(10.0, -6.0 + 4.0 * torch.rand(qv.shape, device=dev)))
            for h in (2.0, 1500.0):
                record(f"pressure_at_height {h:g} m {tag} {lname}", timeit(lambda: native.pressure_at_height_stack(
                       t.data, q.data, sp, Ac, Bc, p, n_pts=n_src, n_lev=L, pitch=t.pitch, layout=layout, height=h)),
                       2 * L * n_src * B + 2 * n_src * B, "q_to_r_height / q_to_d_height: one column walk per point, one log per level")
            del t, q
        torch.cuda.empty_cache()

    def rotate_rows(tdt, B, tag):
        """rotate_winds: u / v stacks of 1 and L levels, both layouts, both frame kinds — algorithmic bytes 4·N·L·B + N·F·B (two
        stacks in, two out, the per-point frame table of F words once)."""
        for n_lev in (1, L):
            for layout, lname in ((COLUMNS, "columns"), (FIELDS, "fields")):
                x, y = Stack.empty(n_src, n_lev, tdt, dev, layout, zero=True), Stack.empty(n_src, n_lev, tdt, dev, layout, zero=True)
                x.data.normal_()
                y.data.normal_()
                xo, yo = x.new_like(), y.new_like()
                for kind, F, kname in ((native.FRAME_ROTATION, 2, "rotation"), (native.FRAME_GENERAL, 4, "general")):
                    frame = torch.rand(n_src, F, dtype=tdt, device=dev)
                    record(f"rotate_vectors {kname} L{n_lev} {tag} {lname}", timeit(lambda: native.rotate_vectors_stack(
                           x.data, y.data, xo.data, yo.data, frame, kind, n_pts=n_src, n_lev=n_lev, pitch=x.pitch, layout=layout)),
                           4 * n_src * n_lev * B + n_src * F * B, "rotate_winds / unrotate_winds: per-point frame, every level")
                del x, y, xo, yo
                torch.cuda.empty_cache()

    def pandas_route_ms(date, cell, values, targets, n_cells, freq_ns):
        """The reference's method for one table on this host, one process: a loop over targets with a groupby().idxmin() in each
        (R: filters/tabular/irregular_to_grid.py:139-159), window (-time_freq, 0], weight 0."""
        try:
            import pandas as pd
        except ImportError:
            return None
        names = [f"v{j}" for j in range(len(values))]
        df = pd.DataFrame({"date": pd.to_datetime(date), "spatial_index": cell, **{n: v for n, v in zip(names, values)}})
        freq = pd.Timedelta(freq_ns, "ns")
        t0 = time.perf_counter()
        grids = {n: np.full((len(targets), n_cells), np.nan) for n in names}
        for t, target in enumerate(pd.to_datetime(targets)):
            part = df[df["date"].gt(target - freq) & df["date"].le(target)]
            part = part[~part[names].isna().all(axis=1)].copy()
            if len(part) == 0:
                continue
            part["_score"] = (part["date"] - target).abs() / freq
            best = part.loc[part.groupby("spatial_index")["_score"].idxmin()]
            index = best["spatial_index"].values.astype(np.intp)
            ok = (index >= 0) & (index < n_cells)
            for n in names:
                grids[n][t, index[ok]] = best[n].values[ok]
        return (time.perf_counter() - t0) * 1e3

    def obs_rows():
        """irregular_to_grid: the keyed arg-min (memsets + score pass + row pass, one entry point) and the fill pass, for rows spread
        uniformly over the cells and for a swath (half the rows in 1 % of the cells: contended atomics).  The fill pass is rated on
        n_time·n_cols·N·8 + n_time·N·4 bytes; the arg-min on what it must read, n_obs·(16 + 8·n_cols) bytes, for orientation only:
        it is bound by scattered atomics, not by bandwidth."""
        hour = 3600 * 10**9
        for gname, n_time, n_cols, n_obs, host_too in (("o96", 4, 4, 1_000_000, True), ("o1280", 8, 8, 20_000_000, False)):
            n_cells = len(lookup(gname)["latitudes"])
            gen = torch.Generator(device=dev).manual_seed(n_obs)
            base = 1_700_000_000 * 10**9
            targets = base + torch.arange(1, n_time + 1, dtype=torch.int64, device=dev) * 6 * hour
            date = base + torch.randint(0, (n_time + 1) * 360, (n_obs,), generator=gen, device=dev) * 60 * 10**9
            values = torch.rand((n_cols, n_obs), dtype=torch.float64, generator=gen, device=dev)
            values[torch.rand((n_cols, n_obs), generator=gen, device=dev) < 0.1] = float("nan")
            uniform = torch.randint(0, n_cells, (n_obs,), generator=gen, device=dev)
            swath = uniform.clone()
            swath[: n_obs // 2] = torch.randint(0, max(1, n_cells // 100), (n_obs // 2,), generator=gen, device=dev)
            swath = swath[torch.randperm(n_obs, generator=gen, device=dev)]
            best = torch.empty((n_time, n_cells), dtype=torch.int64, device=dev)
            winner = torch.empty((n_time, n_cells), dtype=torch.int32, device=dev)
            for cname, cell in (("uniform", uniform), ("swath", swath)):
                shape = f"{gname} T{n_time} C{n_cols} {n_obs:.0e} rows {cname}"
                record(f"obs_best_per_cell {shape}", timeit(lambda: native.obs_best_per_cell(
                       date, cell, values, targets, best, winner, n_cells=n_cells, before_ns=-6 * hour, after_ns=0, closed_before=False,
                       closed_after=True, freq_ns=6 * hour, weight=0.3)), n_obs * (16 + 8 * n_cols),
                       f"two memsets + score pass + row pass; {float((winner >= 0).float().mean()):.3f} of the slots filled")
                for layout, lname in ((COLUMNS, "columns"), (FIELDS, "fields")):
                    out = Stack.empty(n_cells, n_time * n_cols, torch.float64, dev, layout)
                    record(f"obs_fill_stack {shape} {lname}", timeit(lambda: native.obs_fill_stack(
                           winner, values, out.data, n_time=n_time, n_cells=n_cells, pitch=out.pitch, layout=layout)),
                           n_time * n_cols * n_cells * 8 + n_time * n_cells * 4, "gather of 8-byte words by winner, 16-byte non-temporal stores")
                    del out
                if host_too:
                    ms = pandas_route_ms(date.cpu().numpy().view("datetime64[ns]"), cell.cpu().numpy(), values.cpu().numpy(),
                                         targets.cpu().numpy().view("datetime64[ns]"), n_cells, 6 * hour)
                    if ms is not None:
                        res[f"pandas route {shape}"] = {"ms": ms, "note": "the reference's method on this host, one process: per target a "
                                                        "window selection and groupby().idxmin(); the NaN grids it fills stay on the host"}
                        print(f"{'pandas route ' + shape:42s} {ms:9.1f} ms  (host)", flush=True)
            del date, values, uniform, swath, best, winner
            torch.cuda.empty_cache()

    def superob_pandas_ms(table, grid_lat, grid_lon, slot, repeats):
        """The reference's statement for one table on this host, one process, as pandas runs it (R: support/superob.py:43-69,
        superob.py:72-96): cKDTree, groupby().mean(), groupby().idxmin(), concat, sort_values."""
        try:
            import pandas as pd
            from scipy.spatial import cKDTree
        except ImportError:
            return None
        points = np.column_stack([grid_lat, np.where(grid_lon > 180, grid_lon - 360, grid_lon)])
        times = []
        for _ in range(repeats):
            df = pd.DataFrame(table)
            t0 = time.perf_counter()
            df = df.dropna(subset=["date", "latitude", "longitude"])
            time_grid = pd.date_range(df["date"].min(), df["date"].max(), freq=f"{slot}s")
            temporal = np.clip(np.searchsorted(time_grid, df["date"], side="right") - 1, 0, None)
            distances, spatial = cKDTree(points).query(df[["latitude", "longitude"]])
            df = df.assign(grid_index=spatial + len(points) * temporal, spatial_index=spatial, distance=distances)
            keys = ["grid_index", "reportype"]
            averaged = df.groupby(keys, observed=True, sort=False)[[c for c in df.columns if c not in keys + ["date"]]].mean()
            nearest = df.loc[df.groupby(keys, observed=True, sort=False)["distance"].idxmin(), ["date"] + keys].set_index(keys)
            out = pd.concat([averaged, nearest], axis=1, join="inner").reset_index().drop(columns=["grid_index", "distance"])
            out = out.sort_values("date")
            times.append((time.perf_counter() - t0) * 1e3)
            rows = len(out)
            del df, averaged, nearest, out
        return float(np.median(times)), rows

    def superob_rows():
        """superob: the group bookkeeping (torch: fold the keys, one stable sort, segment offsets), the two kernels on their own, and
        the filter end to end — table resident in HBM and table in host memory, interleaved, medians — beside the reference's
        statement in pandas on this host.  4 value columns; mean group sizes 4 and 40; once ONE group of 10^6 rows (its sum is
        sequential by definition).  Algorithmic bytes of bookkeeping + mean: keys (8) + permutation (4) + n_cols * 8 per row in,
        n_cols * 8 per group out; of the mean kernel alone: 4 + n_cols * 8 per row, 8 + n_cols * 16 per group."""
        from anemoi_transform_amd import obs
        from anemoi_transform_amd.filters import create_filter_by_name

        n_cols, slot = 4, 3600
        grid = lookup("o96")
        grid_lat, grid_lon = grid["latitudes"], np.where(grid["longitudes"] > 180, grid["longitudes"] - 360, grid["longitudes"])
        n_grid = len(grid_lat)
        for n, size, single in ((1_000_000, 4, False), (1_000_000, 40, False), (10_000_000, 4, False), (10_000_000, 40, False),
                                (1_000_000, 1_000_000, True)):
            shape = f"{n:.0e} rows C{n_cols} " + ("one group" if single else f"groups of ~{size}")
            rng = np.random.default_rng(n + size)
            n_keys = max(1, n // size)
            n_slots = max(1, round(n_keys / n_grid))
            cell = rng.integers(0, min(n_grid, n_keys), n)
            table = {"date": np.datetime64("2025-01-01T00:00:00", "ns") + rng.integers(0, n_slots * slot, n) * np.timedelta64(10**9, "ns"),
                     "latitude": grid_lat[cell] + rng.uniform(-0.05, 0.05, n), "longitude": grid_lon[cell] + rng.uniform(-0.05, 0.05, n),
                     "reportype": np.full(n, 1001, dtype=np.int64)}
            for j in range(n_cols - 2):  # latitude and longitude are averaged too: n_cols value columns beside spatial_index / distance
                v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
                v[rng.random(n) < 0.1] = np.nan
                table[f"v{j}"] = v
            resident = {k: torch.from_numpy(v.view(np.int64) if v.dtype.kind == "M" else v).to(dev) for k, v in table.items()}
            # the kernels on their own, on the groups the filter forms (cell and slot known here without the search)
            ns = resident["date"]
            key = torch.from_numpy(cell).to(dev) + n_grid * ((ns - ns.min()) // (slot * 10**9))
            values = torch.stack([resident["latitude"], resident["longitude"]] + [resident[f"v{j}"] for j in range(n_cols - 2)])
            distance = torch.rand(n, dtype=torch.float64, device=dev)
            groups = obs.superob_groups([key], None, dev)
            G = groups.n_groups
            mean = torch.empty((n_cols, G), dtype=torch.float64, device=dev)
            count = torch.empty((n_cols, G), dtype=torch.int64, device=dev)
            nearest = torch.empty(G, dtype=torch.int32, device=dev)
            note = f"{G} groups, the largest {int((groups.offsets[1:] - groups.offsets[:-1]).max())} rows"
            t_groups = timeit(lambda: obs.superob_groups([key], None, dev), n=7)
            t_mean = timeit(lambda: native.obs_group_mean(values, groups.order, groups.offsets, mean, count), n=7)
            t_argmin = timeit(lambda: native.obs_group_argmin(distance, groups.order, groups.offsets, nearest), n=7)
            record(f"superob_groups {shape}", t_groups, n * 12, "torch on the device: fold the keys, ONE stable sort, offsets; " + note)
            record(f"obs_group_mean {shape}", t_mean, n * (4 + 8 * n_cols) + G * (8 + 16 * n_cols), "Kahan in row order, lane per (group, column); " + note)
            record(f"obs_group_argmin {shape}", t_argmin, n * 12 + G * 12, "first row of smallest distance; " + note)
            record(f"superob groups + mean {shape}", t_groups + t_mean, n * (12 + 8 * n_cols) + G * 8 * n_cols, "sum of the two rows above")
            res[f"obs_group_mean {shape}"]["rows_per_s"] = n / (t_mean * 1e-3)
            res[f"superob groups + mean {shape}"]["rows_per_s"] = n / ((t_groups + t_mean) * 1e-3)
            del key, values, distance, groups, mean, count, nearest
            # the filter end to end: resident and host-fed interleaved (wall clock around a device synchronise), medians
            f = create_filter_by_name("superob", grid="o96", timeslot_length=slot, columns_to_take_nearest=["date"], columns_to_groupby=["reportype"])
            took = {"resident": [], "host-fed": []}
            for i in range(1 + (3 if n > 2_000_000 else 5)):
                for name, tab in (("resident", resident), ("host-fed", table)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = f(tab)
                    torch.cuda.synchronize()
                    if i:  # the first round warms up (code objects, the grid's search tree)
                        took[name].append((time.perf_counter() - t0) * 1e3)
                    rows_out = len(out["date"])
                    del out
            for name, ts in took.items():
                res[f"superob filter {name} {shape}"] = {"ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "runs": len(ts),
                                                          "rows_per_s": n / (float(np.median(ts)) * 1e-3), "rows_out": rows_out,
                                                          "note": "create_filter_by_name('superob') end to end: drop missing, nearest grid point (device search, "
                                                                  "latitude / longitude and the answer cross the host link), groups, means, nearest row, sort by date"}
                print(f"{'superob filter ' + name + ' ' + shape:58s} {np.median(ts):9.1f} ms  [{min(ts):.1f} .. {max(ts):.1f}]  {rows_out} rows out", flush=True)
            host = superob_pandas_ms(table, grid["latitudes"], grid["longitudes"], slot, repeats=1 if n > 2_000_000 else 3)
            if host is not None:
                res[f"superob pandas {shape}"] = {"ms": host[0], "rows_out": host[1], "runs": 1 if n > 2_000_000 else 3,
                                                  "note": "the reference's statement on this host, one process: cKDTree, groupby().mean(), "
                                                          "groupby().idxmin(), concat, sort_values"}
                print(f"{'superob pandas ' + shape:58s} {host[0]:9.1f} ms  (host)  {host[1]} rows out", flush=True)
            del resident, table
            torch.cuda.empty_cache()

    def checksum(out):
        """Order-sensitive 128-bit checksum of a tensor's bytes, summed on the device in wrapping int64 (of several tensors: one after
        the other); anything else by its repr."""
        if isinstance(out, (list, tuple)):
            return "".join(checksum(o) for o in out)
        if not torch.is_tensor(out):
            return repr(out)
        w = out.contiguous().view(-1).view(torch.int32 if out.element_size() == 4 else (torch.int64 if out.element_size() == 8 else torch.uint8))
        a = b = 0
        for i in range(0, w.numel(), 1 << 26):
            c = w[i:i + (1 << 26)].to(torch.int64)
            a += int(c.sum())
            b += int((c * (torch.arange(i, i + c.numel(), device=c.device) | 1)).sum())
        return f"{a & (2**64 - 1):016x}{b & (2**64 - 1):016x}"

    def pointwise_rows(tdt, B, tag, x=None):
        """The rows that run kernels of atx_pointwise.hip, atx_mask.hip and atx_reduce.hip, on the seeded stack `x` (made here when
        the caller has none).  `digest` is the checksum of what ONE call of the row computes: an in-place row starts from a copy of x."""
        x = x if x is not None else bench.synth_stack(src_grid, L, tdt, dev, 0, COLUMNS)
        y = x.new_like()
        y.data.zero_()  # padding slots are never written: a known value under the checksum
        kw = dict(n_pts=n_src, n_lev=L, x_pitch=x.pitch, y_pitch=y.pitch, layout=COLUMNS)
        stack_bytes = n_src * L * B
        aff, cp = (native.OP_AFFINE, 0, 1.0, -273.15), (native.OP_COPY, 0, 0.0, 0.0)
        pm = (torch.rand(n_src + 8, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) < 0.3).to(torch.uint8)

        def row(name, stages, src, alg_bytes, note="", mask=None):
            prog = native.level_program(stages, dev)
            fn = lambda: native.pointwise_stack(src.data, y.data, prog=prog, n_stage=len(stages), point_mask=mask, **kw)  # noqa: E731
            if src is y:
                y.data.copy_(x.data)
            record(name, timeit(fn), alg_bytes, note)
            if src is y:  # the timed calls compounded: the digest is of one call
                y.data.copy_(x.data)
                fn()
            res[name]["digest"] = checksum(y.data)

        row(f"pointwise affine {tag} out-of-place", [[aff] * L], x, 2 * stack_bytes)
        row(f"pointwise affine {tag} in-place", [[aff] * L], y, 2 * stack_bytes)
        row(f"pointwise 2 stages, uniform over the levels {tag} out-of-place", [[(native.OP_MUL, 0, 9.80665, 0.0)] * L, [aff] * L], x, 2 * stack_bytes,
            "operators by value")
        row(f"pointwise affine, a different operator per level {tag} out-of-place", [[(native.OP_AFFINE, 0, 1.0 + 0.001 * l, -273.15) for l in range(L)]], x,
            2 * stack_bytes, "per-level tables: LDS kernel (f32 out of place), typed no-loop kernel (f64)")
        row(f"pointwise log then exp (sp_to_lnsp | lnsp_to_sp) {tag} out-of-place", [[(native.OP_LOG, 0, 0.0, 0.0)] * L, [(native.OP_EXP, 0, 0.0, 0.0)] * L], x,
            2 * stack_bytes, "log and exp (the library's own routines in float64, atx_common.hpp) on every element")
        row(f"apply_mask {tag}", [[(native.OP_COPY, 1, 0.0, 0.0)] * L], x, 2 * stack_bytes + n_src, mask=pm)
        row(f"pointwise 1 of {L} levels selected {tag} in-place", [[(native.OP_AFFINE, 0, 2.0, 1.0)] + [cp] * (L - 1)], y, 2 * n_src * B,
            "untouched levels are skipped; 16-B vector granularity")
        minmax = lambda: native.reduce_stack(x.data, native.RED_MINMAX, n_pts=n_src, n_lev=L, pitch=x.pitch, layout=COLUMNS)  # noqa: E731
        name = f"reduce min+max of the stack {tag} (one pass)"
        record(name, timeit(minmax), stack_bytes, "the range check of cos_sin_from_rad; includes the device->host read (round 1: two passes of 0.79 ms)")
        res[name]["digest"] = checksum(minmax())
        del y
        f = Stack.empty(n_src, L, tdt, dev, FIELDS)
        native.relayout(x.data, f.data, n_pts=n_src, n_lev=L, src_pitch=x.pitch, dst_pitch=f.pitch, src_layout=COLUMNS, dst_layout=FIELDS)
        g = f.new_like()
        g.data.zero_()
        pf = native.level_program([[(native.OP_AFFINE, 0, 1.0 + 0.001 * l, -273.15) for l in range(L)]], dev)
        name = f"pointwise affine, a scale per field {tag} fields (the reference's array order)"
        record(name, timeit(lambda: native.pointwise_stack(f.data, g.data, prog=pf, n_stage=1, n_pts=n_src, n_lev=L, x_pitch=f.pitch, y_pitch=g.pitch, layout=FIELDS)),
               2 * stack_bytes, "one vector per lane, grid.y = field")
        res[name]["digest"] = checksum(g.data)
        first = f.data[0].contiguous()
        mask = torch.zeros(n_src + 8, dtype=torch.uint8, device=dev)
        name = f"mask_build {tag} (1 field)"
        record(name, timeit(lambda: native.mask_build(first, mask, n=n_src, cmp=native.CMP_GT, threshold=280.0)), n_src * (B + 1))
        res[name]["digest"] = checksum(mask)
        name = f"reduce min {tag} (1 field)"
        record(name, timeit(lambda: native.reduce(first, native.RED_MIN)), n_src * B, "includes the device->host read of the result")
        res[name]["digest"] = checksum(native.reduce(first, native.RED_MIN))
        if B == 8:  # once per table
            m = (torch.rand(n_src, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) < 0.7).to(torch.uint8)
            name = "mask_to_index (6.6M points, 70% kept)"
            record(name, timeit(lambda: native.mask_to_index(m, n_src)), 2 * n_src + 4 * int(m.sum().item()), "includes workspace allocation + count read-back")
            res[name]["digest"] = checksum(native.mask_to_index(m, n_src))
        del f, g
        torch.cuda.empty_cache()

    def side_by_side(rows, libs, rounds):
        """rows: (name, call, one_call, algorithmic bytes, note).  Every library times every row in each of `rounds` rounds, one process,
        after one round that is thrown away (code objects, clocks), the libraries alternating and taking turns to go first; the
        per-round medians go to `<name>_ms`, and the digests of one_call() must agree."""
        times = {(name, lib): [] for name, *_ in rows for lib in libs}
        before = native.use_library(None)
        for r in range(rounds + 1):
            for lib in (list(libs) if r % 2 else list(libs)[::-1]):
                native.use_library(libs[lib])
                for name, call, *_ in rows:
                    ms = timeit(call)
                    if r:  # round 0 warms up
                        times[name, lib].append(ms)
        for name, call, one_call, alg_bytes, note in rows:
            digests = {}
            for lib, handle in libs.items():
                native.use_library(handle)
                digests[lib] = checksum(one_call())
            ref, *others = libs
            lo, hi = min(times[name, ref]), max(times[name, ref])
            res[name] = {"algorithmic_bytes": alg_bytes, "note": note, "digest": digests[ref], "digests_equal": len(set(digests.values())) == 1}
            line = f"{name:74s}"
            for lib in libs:
                med = float(np.median(times[name, lib]))
                res[name][f"{lib}_ms"] = times[name, lib]
                res[name][f"{lib}_median_ms"] = med
                line += f" {lib} {med:8.4f}"
            for lib in others:
                med = res[name][f"{lib}_median_ms"]
                res[name][f"{lib}_minus_{ref}_pct"] = 100.0 * (med / res[name][f"{ref}_median_ms"] - 1.0)
                res[name][f"{lib}_within_{ref}_spread"] = bool(lo <= med <= hi)
                line += f"  {res[name][f'{lib}_minus_{ref}_pct']:+5.2f} %  in [{lo:.4f}, {hi:.4f}]: {lo <= med <= hi}"
            print(line + ("" if res[name]["digests_equal"] else "  DIGESTS DIFFER"), flush=True)
        native.use_library(before)

    def regrid_rows(tdt, B, tag, x, idx, w, libs=None, rounds=1):
        """The rows that run kernels of atx_regrid_columns.inc and atx_regrid_fields.inc, on the seeded stack `x`.  `digest` is the
        checksum of what ONE call of the row writes into an output stack zeroed first (padding slots are never written).  With
        `libs` ({name: handle}, the first one the reference): side_by_side() over all rows.  (This mode keeps every plan alive until the end.)"""
        from anemoi_transform_amd.gather import target_order_for

        rows = []

        def row(name, plan, alg_bytes, note="", src=x, tile=0, **kw):
            def call(out=None):
                native.set_tuning(tile)
                try:
                    return plan.apply(src, out=out, **kw)
                finally:
                    native.set_tuning(0)

            def one_call():
                out = Stack.empty(plan.n_tgt, L, tdt, dev, src.layout, zero=True)
                return call(out).data

            if libs:
                rows.append((name, call, one_call, alg_bytes, note))
            else:  # measured here, so that a plan the caller does not keep is freed before the next one is built
                record(name, timeit(call), alg_bytes, note)
                res[name]["digest"] = checksum(one_call())

        U4, U1 = int(np.unique(idx).size), int(np.unique(idx[:, 0]).size)
        plan4 = GatherPlan(n_src, n_tgt, index=idx, weights=w)
        plan1 = GatherPlan(n_src, n_tgt, index=idx[:, 0])
        row(f"regrid_ell k=4 {tag} columns", plan4, bench.algorithmic_bytes(L, B, U4, n_tgt, 4), "incl. output allocation")
        row(f"regrid_ell k=1 {tag} columns", plan1, bench.algorithmic_bytes(L, B, U1, n_tgt, 1))
        keep = (np.arange(idx.size) % 9 != 0).reshape(idx.shape)
        indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
        csr = GatherPlan(n_src, n_tgt, csr=(w[keep], idx[keep], indptr))
        nnz = int(keep.sum())
        csr_bytes = L * B * (int(np.unique(idx[keep]).size) + n_tgt) + nnz * (4 + B) + 4 * n_tgt
        row(f"regrid_csr ragged(3-4) {tag} columns", csr, csr_bytes, "general CSR kernel")
        padded = GatherPlan.from_matrix(dict(matrix_data=w[keep], matrix_indices=idx[keep], matrix_indptr=indptr, matrix_shape=(n_tgt, n_src)))
        assert padded.padded
        row(f"regrid ragged(3-4) as padded fixed-k {tag}", padded, csr_bytes, "what regrid(matrix=...) uses for short ragged rows")
        tile = 16 if B == 4 else 8  # what the tiled kernels' heuristic picks at 137 levels
        row(f"regrid_csr ragged(3-4) {tag} columns, TILED kernel", csr, csr_bytes, "round 1's kernel (LDS-staged CSR slice)", tile=tile)
        # long rows: 16 nearest neighbours, and the same with entries dropped (rows of 9-16)
        idx16, w16 = interp.knn_inverse_distance(src_grid, tgt_grid, k=16, device=True, ties="index")
        U16 = int(np.unique(idx16).size)
        blocks16, blocks12 = (target_order_for(tgt_grid["latitudes"], tgt_grid["longitudes"], k) for k in (16, 12))
        bytes16 = bench.algorithmic_bytes(L, B, U16, n_tgt, 16)
        row(f"regrid_ell k=16 {tag} columns", GatherPlan(n_src, n_tgt, index=idx16, weights=w16), bytes16,
            "compile-time k = 16 on the direct kernel; targets in natural order, workgroups dealt to the XCDs in stripes (round 4)")
        row(f"regrid_ell k=16 {tag} columns, targets in column blocks", GatherPlan(n_src, n_tgt, index=idx16, weights=w16).order_targets(blocks16), bytes16,
            "what regrid(matrix=...) does for k >= 5 on large output grids (atx_regrid_ell_ordered; same bits)")
        rng16 = np.random.default_rng(16)
        keep16 = rng16.random(idx16.shape) < 0.75
        keep16[:, :9] = True
        indptr16 = np.concatenate([[0], np.cumsum(keep16.sum(axis=1))])
        csr16_tables = (w16[keep16], idx16[keep16], indptr16)
        csr16 = GatherPlan(n_src, n_tgt, csr=csr16_tables)
        nnz16 = int(keep16.sum())
        csr16_bytes = L * B * (int(np.unique(idx16[keep16]).size) + n_tgt) + nnz16 * (4 + B) + 4 * n_tgt
        row(f"regrid_csr rows of 9-16 {tag} columns", csr16, csr16_bytes, "general CSR, direct kernel")
        row(f"regrid_csr rows of 9-16 {tag} columns, TILED kernel", csr16, csr16_bytes, "round 1's kernel", tile=tile)
        matrix16 = dict(matrix_data=csr16_tables[0], matrix_indices=csr16_tables[1], matrix_indptr=indptr16, matrix_shape=(n_tgt, n_src))
        padded16 = GatherPlan.from_matrix(matrix16)
        assert padded16.padded and padded16.k == 16
        row(f"regrid rows of 9-16 as padded fixed-k {tag}", padded16, csr16_bytes, "what regrid(matrix=...) uses for ragged rows up to 16 entries")
        row(f"regrid rows of 9-16 as padded fixed-k {tag}, targets in column blocks", GatherPlan.from_matrix(matrix16).order_targets(blocks16), csr16_bytes,
            "the same in the order the regrid filter's policy picks on large output grids")
        row(f"regrid_csr rows of 9-16 {tag} columns, targets in column blocks", GatherPlan(n_src, n_tgt, csr=csr16_tables).order_targets(blocks12), csr16_bytes,
            "what regrid(matrix=...) does for long ragged rows on large output grids (atx_regrid_csr_ordered; same bits)")
        del csr16, padded16
        # coarsening by box averages (a conservative-style matrix): every 1-degree cell averages the ~200 O1280 points inside it
        one = lookup([1.0, 1.0])
        n_one = len(one["latitudes"])
        cell = (np.rint(90.0 - src_grid["latitudes"]).astype(np.int64) * 360 + np.mod(np.rint(src_grid["longitudes"]).astype(np.int64), 360))
        order_b = np.argsort(cell, kind="stable")
        counts_b = np.bincount(cell, minlength=n_one)
        indptr_b = np.concatenate([[0], np.cumsum(counts_b)])
        data_b = (1.0 / np.maximum(counts_b, 1))[cell[order_b]]
        box_bytes = L * B * (n_src + n_one) + n_src * (4 + B) + 4 * n_one
        row(f"regrid_csr box average O1280->1deg {tag} (rows of ~{int(counts_b.mean())})", GatherPlan(n_src, n_one, csr=(data_b, order_b.astype(np.int32), indptr_b)),
            box_bytes, "general CSR, every source column read once")
        prog = native.level_program([[(native.OP_MUL, 0, 9.80665, 0.0)] * L, [(native.OP_AFFINE, 0, 1.0, -273.15)] * L], dev)
        row(f"regrid_ell k=4 {tag} + 2-stage epilogue", plan4, bench.algorithmic_bytes(L, B, U4, n_tgt, 4), "fused regrid -> orog_to_z -> rescale, every level",
            prog=prog, n_stage=2)
        cp = (native.OP_COPY, 0, 0.0, 0.0)
        prog5 = native.level_program([[cp] * (L - 1) + [(native.OP_MUL, 0, 9.80665, 0.0)], [(native.OP_AFFINE, 0, 1.0, -273.15)] * (L - 1) + [cp]], dev)
        row(f"regrid_ell k=4 {tag} + config-5 epilogue", plan4, bench.algorithmic_bytes(L, B, U4, n_tgt, 4),
            "136 levels convert, 1 level orog_to_z: operators by value, two pieces", prog=prog5, n_stage=2)
        # ---- regrid on field-major
        f = Stack.empty(n_src, L, tdt, dev, FIELDS)
        native.relayout(x.data, f.data, n_pts=n_src, n_lev=L, src_pitch=x.pitch, dst_pitch=f.pitch, src_layout=COLUMNS, dst_layout=FIELDS)
        row(f"regrid_ell k=4 {tag} fields", plan4, bench.algorithmic_bytes(L, B, U4, n_tgt, 4), src=f)

        if not libs:
            return
        side_by_side(rows, libs, rounds)

    def combine_rows(tdt, B, tag, x, libs=None, rounds=1):
        """The rows that run kernels of atx_combine.hip and atx_relayout.hip (multi-input operators, layout conversion, level
        selection), on the seeded stack `x`.  `digest` is the checksum of what ONE call of the row writes into outputs zeroed first.
        With `libs`: side_by_side() over each block of rows as it comes, so that a block's operands are freed before the next one's."""
        gen = torch.Generator(device=dev).manual_seed(L)
        rand = lambda *shape: torch.rand(shape, device=dev, generator=gen)  # noqa: E731
        stack_bytes = n_src * L * B
        rows = []

        def row(name, fn, outs, alg_bytes, note=""):
            def one_call():
                for o in outs:
                    o.zero_()
                fn()
                return outs

            rows.append((name, fn, one_call, alg_bytes, note))

        def combine(name, op, ins, outs, alg_bytes, note="", n_lev=L, **kw):
            row(f"combine {name} {tag}", lambda: native.combine_stack(op, ins, outs, n_pts=n_src, n_lev=n_lev, pitch=outs[0].stride(0), layout=COLUMNS, **kw),
                outs, alg_bytes, note)

        def finish():
            if libs:
                side_by_side(rows, libs, rounds)
            else:
                for name, fn, one_call, alg_bytes, note in rows:
                    record(name, timeit(fn), alg_bytes, note)
                    res[name]["digest"] = checksum(one_call())
            rows.clear()
            torch.cuda.empty_cache()

        y, z = x.new_like(), x.new_like()
        y.data.copy_(x.data)
        # snow depth (m of water equivalent) and density as they occur — in REGIONS, as on a real field (points are stored by
        # latitude): ~55 % of the points bare (sd = 0), ~35 % deep snow, ~10 % a thin cover where tanh really has to be evaluated;
        # density 100-400 kg/m3
        sd, thin, rsn = x.new_like(), x.new_like(), x.new_like()
        u = (torch.arange(n_src, device=dev, dtype=torch.float64) / n_src).unsqueeze(1).expand(n_src, L)
        sd.data[:, :L] = torch.where(u < 0.55, torch.zeros_like(u), torch.where(u < 0.9, 0.05 + u, 1e-4 * u)).to(tdt)
        rsn.data[:, :L] = (100.0 + 300.0 * rand(n_src, L)).to(tdt)
        thin.data.fill_(1e-5)  # 4000 * (1000 * 1e-5 / rsn) / rsn < 2.65 everywhere: tanh on every element
        del u
        combine("snow_cover (2->1)", native.COMB_SNOW_COVER, [sd.data, rsn.data], [z.data], 3 * stack_bytes, "regions: 55 % bare, 35 % deep snow, 10 % thin cover (tanh evaluated)")
        combine("snow_cover (2->1), thin cover everywhere", native.COMB_SNOW_COVER, [thin.data, rsn.data], [z.data], 3 * stack_bytes, "worst case: tanh evaluated on every element")
        combine("difference (2->1, accum_to_interval)", native.COMB_SUB, [x.data, y.data], [z.data], 3 * stack_bytes)
        finish()
        del sd, thin, rsn
        combine("cos_sin (1->2)", native.COMB_COS_SIN, [x.data], [y.data, z.data], 3 * stack_bytes)
        finish()  # (y holds cos x from here on)
        # ---- the numpy-only domain filters (filters/domain.py)
        lim = torch.full((L,), 10000.0, dtype=torch.float64, device=dev)
        w2, dm = x.new_like(), x.new_like()
        dm.data[:, :L] = torch.randint(0, 4, (n_src, L), device=dev, generator=gen).to(tdt)
        combine("opera_clipping (2->2)", native.COMB_OPERA_CLIP, [x.data, y.data], [z.data, w2.data], 4 * stack_bytes, level_param=lim)
        combine("opera_preprocessing (3->2)", native.COMB_OPERA_PREPROCESS, [x.data, y.data, dm.data], [z.data, w2.data], 5 * stack_bytes, level_param=lim)
        finish()
        del dm, w2
        # humidity conversions: q in [1e-6, 2e-2], t in [190, 320] K — water, mixed and ice branches of the saturation curve all present
        qh, th = x.new_like(), x.new_like()
        qh.data[:, :L] = (10.0 ** (-6.0 + 4.3 * rand(n_src, L))).to(tdt)
        th.data[:, :L] = (190.0 + 130.0 * rand(n_src, L)).to(tdt)
        plev = torch.linspace(1.0, 1000.0, L, dtype=torch.float64, device=dev)
        combine("q_to_r (2->1)", native.COMB_Q_TO_R, [qh.data, th.data], [z.data], 3 * stack_bytes, "one or two exp per element (mixed phase)", level_param=plev)
        combine("r_to_d (2->1)", native.COMB_R_TO_D, [y.data, th.data], [z.data], 3 * stack_bytes, "one exp and one log per element")
        finish()
        del qh, th
        # one ORAS6 group: 14 fields and the ice concentration they share
        o_in, o_out = Stack.empty(n_src, 14, tdt, dev, COLUMNS), Stack.empty(n_src, 14, tdt, dev, COLUMNS)
        o_in.data.copy_(torch.randn(o_in.data.shape, device=dev, generator=gen))
        ice = rand(n_src).to(tdt)
        kinds = torch.tensor([0, 1, 1, 1, 4, 4, 1, 2, 3, 1, 1, 1, 2, 5], dtype=torch.float64, device=dev)
        combine("oras6_clipping (14 fields of one date)", native.COMB_ORAS6, [o_in.data, ice], [o_out.data], (2 * 14 + 1) * n_src * B,
                "one launch per group; the shared ice field is read once per point", n_lev=14, level_param=kinds)
        cls = Stack.empty(n_src, 1, tdt, dev, COLUMNS)
        cls.data[:, 0] = torch.randint(0, 21, (n_src,), device=dev, generator=gen).to(tdt)
        val = cls.new_like()
        tab = torch.tensor([21.0] + [float(i) for i in range(21)], dtype=torch.float64, device=dev)
        combine("lookup (land_parameters, 1 field)", native.COMB_LOOKUP, [cls.data], [val.data], 2 * n_src * B, "26 MB / 53 MB: launch-latency sized", n_lev=1, level_param=tab)
        finish()
        del o_in, o_out, ice, cls, val, z
        # ---- layout
        f = Stack.empty(n_src, L, tdt, dev, FIELDS)
        row(f"relayout columns->fields {tag}", lambda: native.relayout(x.data, f.data, n_pts=n_src, n_lev=L, src_pitch=x.pitch, dst_pitch=f.pitch,
            src_layout=COLUMNS, dst_layout=FIELDS), [f.data], 2 * stack_bytes)
        finish()  # (f holds x from here on)
        row(f"relayout fields->columns {tag}", lambda: native.relayout(f.data, y.data, n_pts=n_src, n_lev=L, src_pitch=f.pitch, dst_pitch=y.pitch,
            src_layout=FIELDS, dst_layout=COLUMNS), [y.data], 2 * stack_bytes)
        # ---- level gather (re-listing / sub-selecting the fields of a stack, operand stacks of the multi-input filters)
        half, one_lev = Stack.empty(n_src, 68, tdt, dev, COLUMNS), Stack.empty(n_src, 1, tdt, dev, COLUMNS)
        row(f"select 68 of {L} levels (every other one) {tag}", lambda: native.select_levels(x.data, half.data, list(range(0, L - 1, 2)), n_pts=n_src, n_src_lev=L,
            src_pitch=x.pitch, dst_pitch=half.pitch, layout=COLUMNS), [half.data], 2 * n_src * 68 * B, "atx_select_levels; the source lines are read whole: 3x the algorithmic bytes")
        row(f"select 1 of {L} levels {tag}", lambda: native.select_levels(x.data, one_lev.data, [77], n_pts=n_src, n_src_lev=L, src_pitch=x.pitch,
            dst_pitch=one_lev.pitch, layout=COLUMNS), [one_lev.data], 2 * n_src * B, "one field out of a column stack: a 64-byte sector per point is the least that can move")
        finish()

    if args.only_combine:
        libs = {name: native.open_library(os.path.abspath(path), older_build=True) for name, path in (spec.split("=", 1) for spec in args.lib)}
        for tdt, B, tag in ((torch.float32, 4, "f32"), (torch.float64, 8, "f64")):
            combine_rows(tdt, B, tag, bench.synth_stack(src_grid, L, tdt, dev, 0, COLUMNS), libs, args.rounds)
            torch.cuda.empty_cache()
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return

    if args.only_regrid:
        libs = {name: native.open_library(os.path.abspath(path), older_build=True) for name, path in (spec.split("=", 1) for spec in args.lib)}
        idx, w = interp.knn_inverse_distance(src_grid, tgt_grid, k=4)
        for tdt, B, tag in ((torch.float32, 4, "f32"), (torch.float64, 8, "f64")):
            regrid_rows(tdt, B, tag, bench.synth_stack(src_grid, L, tdt, dev, 0, COLUMNS), idx, w, libs, args.rounds)
            torch.cuda.empty_cache()
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return

    if args.only_pointwise:
        for tdt, B, tag in ((torch.float32, 4, "f32"), (torch.float64, 8, "f64")):
            pointwise_rows(tdt, B, tag)
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return

    def rowops_rows():
        """The three per-row observation kernels at args.rows rows, once each: rows/s and the fraction of the HBM peak on algorithmic
        bytes (they are VALU-bound: the fraction says how far from the memory roof the arithmetic keeps them), beside the reference's
        numpy statements (tests/obs_rowops_restatement.py) on this host, one process, at a tenth of the rows."""
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import obs_rowops_restatement as R
        from anemoi_transform_amd import obs

        n = args.rows
        rng = np.random.default_rng(n)
        date = R.random_dates(rng, n)
        lat, lon = rng.uniform(-90.0, 90.0, n), rng.uniform(-180.0, 360.0, n)
        sat_lon = rng.choice([0.0, 41.5, 45.5, -3.4], n)
        n_ch = 4
        channels = np.array([7, 714, 1000, 2211])
        radiance = 10.0 ** rng.uniform(-3.0, 2.5, (n_ch, n))
        d_date, d_lat, d_lon, d_sat_lon, d_rad = (torch.from_numpy(a).to(dev) for a in (date, lat, lon, sat_lon, radiance))
        d_sat_lat = torch.zeros(n, dtype=torch.float64, device=dev)
        a, b = (torch.from_numpy(t).to(dev) for t in R.planck_tables(channels, "cris_fsr"))
        out9 = torch.empty((9, n), dtype=torch.float64, device=dev)
        out2 = torch.empty((2, n), dtype=torch.float64, device=dev)
        out_bt = torch.empty_like(d_rad)
        m = n // 10
        host = {}
        for name, fn in (("forcings", lambda: R.forcings(date[:m], lat[:m], lon[:m], list(R.FORCINGS))),
                         ("view_angles", lambda: (R.calc_azimuth(lat[:m], lon[:m], np.zeros(m), sat_lon[:m]), R.calc_zenith(lat[:m], lon[:m], np.zeros(m), sat_lon[:m]))),
                         ("planck_bt", lambda: R.brightness_temperature(radiance[:, :m].T, *R.planck_tables(channels, "cris_fsr")))):
            t0 = time.perf_counter()
            fn()
            host[name] = m / (time.perf_counter() - t0)
        rows = (("obs_forcings 9 columns", "forcings", lambda: native.obs_forcings(d_date, d_lat, d_lon, 0x1ff, out9), n * (24 + 72), n,
                 "all nine forcings in one pass: julian day, hours and the angles once per row"),
                ("obs_view_angles azimuth + zenith", "view_angles", lambda: native.obs_view_angles(d_lat, d_lon, d_sat_lat, d_sat_lon, 3, out2), n * (32 + 16), n,
                 "both angles in one pass: the sines and cosines of the four positions shared"),
                (f"obs_planck_bt {n_ch} channels", "planck_bt", lambda: native.obs_planck_bt(d_rad, a, b, out_bt), n * n_ch * 16, n,
                 "b / log1p(a / max(R * 1e-2, 1e-300)), blockIdx.y = channel"))
        for name, key, fn, alg, n_rows, note in rows:
            ms = timeit(fn, n=9)
            label = f"{name} {n:.0e} rows"
            record(label, ms, alg, note)
            res[label].update(rows_per_s=n_rows / (ms * 1e-3), numpy_rows_per_s=host[key], numpy_rows=m, commit=args.commit)
            print(f"{'':42s} {n_rows / (ms * 1e-3):.3e} rows/s; numpy on this host, one process, {m} rows: {host[key]:.3e} rows/s", flush=True)

    def healpix_rows():
        """atx_healpix_ang2pix at args.rows rows: rows/s and the fraction of the HBM peak on its 24 algorithmic bytes per row (it is
        VALU-bound: one float64 sincos, an fmod and a sqrt per row), beside the vectorised numpy restatement
        (tests/healpix_restatement.py) on this host, one process, at a tenth of the rows."""
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import healpix_restatement as R

        n = args.rows
        lon, lat = R.random_rows(n, seed=n)
        d_lon, d_lat = torch.from_numpy(lon).to(dev), torch.from_numpy(lat).to(dev)
        out = torch.empty(n, dtype=torch.int64, device=dev)
        n_bad = torch.zeros(1, dtype=torch.int64, device=dev)
        m = n // 10
        for nside, nest in ((32, True), (1 << 29, True), (32, False)):
            t0 = time.perf_counter()
            want = R.ang2pix(nside, lon[:m], lat[:m], nest)
            host = m / (time.perf_counter() - t0)
            ms = timeit(lambda: native.healpix_ang2pix(d_lon, d_lat, nside, nest, out, n_bad), n=9)
            differ = int((out[:m].cpu().numpy() != want).sum())  # rows on a pixel edge, where the last bit of cos / sin decides
            label = f"healpix_ang2pix {'nest' if nest else 'ring'} nside {nside} {n:.0e} rows"
            record(label, ms, n * 24, "one sincos, one fmod and one sqrt per row; two columns in, one out")
            res[label].update(rows_per_s=n / (ms * 1e-3), numpy_rows_per_s=host, numpy_rows=m, rows_unlike_numpy=differ, n_bad=int(n_bad.item()),
                              commit=args.commit)
            print(f"{'':42s} {n / (ms * 1e-3):.3e} rows/s; numpy on this host, one process, {m} rows: {host:.3e} rows/s; {differ} of {m} rows "
                  "differ from numpy's", flush=True)

    def fill_heights_rows():
        """atx_obs_fill_heights at args.rows rows against a 1801 x 3600 float32 orography (0.1 degrees, 26 MB), half of the rows to
        fill — beside the restatement (one cKDTree per axis and fancy indexing, tests/fill_heights_restatement.py) on this host, one
        process, at a tenth of the rows.  Three more rows take the kernel apart with EVERY row to fill: against a 2 x 2 orography (one
        search step per axis, four heights: the row traffic and the counters alone), against the full orography with all rows inside
        one cell (full-depth searches whose reads are the same for every lane, one cache line of heights) and with rows anywhere
        (scattered axis reads and the random gather on top)."""
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import fill_heights_restatement as R
        from anemoi_transform_amd import obs

        n = args.rows
        rng = np.random.default_rng(n)
        lat_axis, lon_axis = np.linspace(90.0, -90.0, 1801), np.arange(3600) * 0.1  # north to south, as orography files come
        h = R.heights(1801, 3600, np.float32)
        grid = obs.HeightGrid(lat_axis, lon_axis, h, dev)
        small = obs.HeightGrid(np.array([-45.0, 45.0]), np.array([0.0, 180.0]), np.arange(4, dtype=np.float32).reshape(2, 2), dev)
        lat, lon = rng.uniform(-90.0, 90.0, n), rng.uniform(0.0, 360.0, n)
        alt = rng.uniform(-400.0, 8800.0, n)
        alt[rng.random(n) < 0.5] = np.nan
        m = max(n // 10, 1)
        t0 = time.perf_counter()
        want = R.fill(lat_axis, lon_axis, h, lat[:m], lon[:m], alt[:m])
        host = m / (time.perf_counter() - t0)
        d_lat, d_lon, d_alt = (torch.from_numpy(a).to(dev) for a in (lat, lon, alt))
        d_nan = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        d_lat1, d_lon1 = (torch.from_numpy(a).to(dev) for a in (rng.uniform(12.26, 12.34, n), rng.uniform(77.06, 77.14, n)))
        out = torch.empty(n, dtype=torch.float64, device=dev)
        flags = torch.empty(n, dtype=torch.uint8, device=dev)
        counters = torch.zeros(3, dtype=torch.int64, device=dev)

        def run(g, la, lo, al, order=None):
            order = g.d_order if order is None else order
            return lambda: native.obs_fill_heights(la, lo, al, g.d_sorted[0], order[0], g.d_sorted[1], order[1], g.heights, out, flags, counters)

        first = tuple(torch.zeros_like(o) for o in grid.d_order)  # every row gathers heights[0, 0]: the searches without the gather

        for label, call, note in (
                (f"fill_heights 1801x3600 f32 {n:.0e} rows, half to fill", run(grid, d_lat, d_lon, d_alt), "the flagship shape"),
                (f"fill_heights 2x2 f32 {n:.0e} rows, all to fill", run(small, d_lat, d_lon, d_nan), "row traffic and counters alone"),
                (f"fill_heights 1801x3600 f32 {n:.0e} rows, all to fill in one cell", run(grid, d_lat1, d_lon1, d_nan),
                 "plus two full-depth searches with lane-uniform reads; one line of heights"),
                (f"fill_heights 1801x3600 f32 {n:.0e} rows, all to fill anywhere, gather from one element", run(grid, d_lat, d_lon, d_nan, first),
                 "the searches read the axes at scattered positions; permutations zeroed, so every gather reads heights[0, 0]"),
                (f"fill_heights 1801x3600 f32 {n:.0e} rows, all to fill anywhere", run(grid, d_lat, d_lon, d_nan),
                 "plus the random gather")):
            ms = timeit(call, n=9)
            filled, flagged, bad = counters.cpu().tolist()
            record(label, ms, n * 33, f"{note}; three columns in, one column and one flag byte out")
            res[label].update(rows_per_s=n / (ms * 1e-3), filled=filled, flagged=flagged, not_finite=bad, commit=args.commit)
            print(f"{'':42s} {n / (ms * 1e-3):.3e} rows/s; {filled} filled, {flagged} flagged", flush=True)
        label = f"fill_heights 1801x3600 f32 {n:.0e} rows, half to fill"
        got = obs.fill_heights(grid, d_lat[:m], d_lon[:m], d_alt[:m]).cpu().numpy()
        differ = int((got.view(np.int64) != want.view(np.int64)).sum())
        res[label].update(scipy_rows_per_s=host, scipy_rows=m, rows_unlike_scipy=differ)
        print(f"{'':42s} cKDTree + fancy indexing on this host, one process, {m} rows: {host:.3e} rows/s; {differ} of {m} rows differ", flush=True)

    if args.only_fill_heights:
        fill_heights_rows()
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return

    if args.only_healpix:
        healpix_rows()
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return

    if args.only_rowops:
        rowops_rows()
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return

    if args.only_superob:
        superob_rows()
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return

    if args.only_obs:
        obs_rows()
        superob_rows()
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return

    if args.only_rotate:
        for tdt, B, tag in ((torch.float32, 4, "f32"), (torch.float64, 8, "f64")):
            rotate_rows(tdt, B, tag)
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return

    if args.only_vertical:
        for tdt, B, tag in ((torch.float32, 4, "f32"), (torch.float64, 8, "f64")):
            vertical_rows(tdt, B, tag)
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return

    idx, w = interp.knn_inverse_distance(src_grid, tgt_grid, k=4)
    for tdt, npdt, B, tag in ((torch.float32, np.float32, 4, "f32"), (torch.float64, np.float64, 8, "f64")):
        vertical_rows(tdt, B, tag)
        rotate_rows(tdt, B, tag)
        x = bench.synth_stack(src_grid, L, tdt, dev, 0, COLUMNS)
        regrid_rows(tdt, B, tag, x, idx, w)
        # ---- per-point
        y = x.new_like()
        record(f"(ceiling) torch copy_ of the stack {tag}", timeit(lambda: y.data.copy_(x.data)), 2 * x.data.numel() * B,
               "device-to-device copy of the same bytes: the practical read+write streaming rate")
        pointwise_rows(tdt, B, tag, x)
        del y
        combine_rows(tdt, B, tag, x)
        del x
        torch.cuda.empty_cache()

    # ---- k-NN precompute
    sxyz = torch.from_numpy(np.ascontiguousarray(interp.unit_sphere_xyz(src_grid["latitudes"], src_grid["longitudes"]))).to(dev)
    txyz = torch.from_numpy(np.ascontiguousarray(interp.unit_sphere_xyz(tgt_grid["latitudes"], tgt_grid["longitudes"]))).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = native.KnnIndex(sxyz)
    torch.cuda.synchronize()
    res["knn_build O1280"] = {"ms": (time.perf_counter() - t0) * 1e3}
    for k in (1, 4):
        res[f"knn_query O1280->0.25 k={k}"] = {"ms": timeit(lambda: index.query(txyz, k), n=3, warm=1)}
    print({k: v for k, v in res.items() if k.startswith("knn")})
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
