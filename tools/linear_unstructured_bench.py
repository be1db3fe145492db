"""Linear regridding from unstructured source grids at working sizes: what the point location costs on the device and on the host.

    python tools/linear_unstructured_bench.py --json profiles/linear_unstructured_bench.json

For O96 -> 1 degree and a limited-area grid of ~10^6 points (0.02 degree, 1000 x 1000, 40-60 N, 0-20 E; targets: 800 x 800 points at
0.0225 degree inside it, edge limit 3 grid spacings) it records
  - the hull (``interp.triangulate_sphere``, host, Qhull, wall clock), triangles and flagged triangles;
  - the kernel ``atx_mesh_locate`` alone on a resident mesh and resident seeds — device events after warming, ``--reps`` runs, the median
    with the smallest and the largest — with the mean and the largest number of moves and the status counts;
  - the seed search (``atx_knn_build`` + ``atx_knn_query`` over the hull vertices) the same way;
  - the host walk ``interp.locate_walk_host`` on the same seeds (one run, wall clock) and that the kernel's four outputs equal it;
  - the whole build as a caller sees it, ``interp.linear_triangulated(device=True)`` and ``device=False`` (wall clock, hull included),
    that the two matrices are equal bit for bit, and the share of rows that the host decided (status 1 after the kernel).
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
from anemoi_transform_amd import interp, native, native_mesh  # noqa: E402
from anemoi_transform_amd.grids import lookup  # noqa: E402
from anemoi_transform_amd.spatial import R_earth_km  # noqa: E402


def box(lat0, lat1, n_lat, lon0, lon1, n_lon):
    lat, lon = np.meshgrid(np.linspace(lat1, lat0, n_lat), np.linspace(lon0, lon1, n_lon), indexing="ij")
    return dict(latitudes=lat.reshape(-1), longitudes=lon.reshape(-1))


CASES = {
    "O96->1deg": (lambda: lookup("o96"), lambda: lookup([1.0, 1.0]), None),
    "lam-1000x1000->800x800": (lambda: box(40.0, 60.0, 1000, 0.0, 20.0, 1000), lambda: box(41.0, 59.0, 800, 1.0, 19.0, 800),
                               3 * np.deg2rad(20.0 / 999) * R_earth_km),
}


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


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def run(name: str, dev, reps: int) -> dict:
    src_of, tgt_of, max_edge_km = CASES[name]
    src, tgt = src_of(), tgt_of()
    src_xyz, tgt_xyz = interp._grid_xyz(src, "in_grid"), interp._grid_xyz(tgt, "out_grid")
    max_edge = None if max_edge_km is None else 2.0 * np.sin(max_edge_km / R_earth_km / 2.0)
    mesh, hull_s = wall(lambda: interp.triangulate_sphere(src_xyz, max_edge))
    hull = mesh["hull_vertices"]
    row = dict(case=name, n_src=len(src_xyz), n_tgt=len(tgt_xyz), max_edge_km=max_edge_km, hull_s=hull_s, triangles=len(mesh["tri"]),
               flagged=int(mesh["flag"].sum()), hull_vertices=len(hull))

    src_d, tgt_d = torch.from_numpy(src_xyz).to(dev), torch.from_numpy(tgt_xyz).to(dev)
    hull_xyz_d = src_d[torch.from_numpy(hull).to(dev)].contiguous()
    row["seed_search"] = device_events(lambda: native.KnnIndex(hull_xyz_d).query(tgt_d, 1), reps)
    nearest, _ = native.KnnIndex(hull_xyz_d).query(tgt_d, 1)
    seed = mesh["vertex_tri"][hull[nearest[:, 0].cpu().numpy()]]
    seed_d = torch.from_numpy(seed).to(dev)
    on_device = native_mesh.Mesh(src_d, *(torch.from_numpy(mesh[k]).to(dev) for k in ("tri", "nbr", "flag")))
    row["kernel"] = device_events(lambda: native_mesh.locate(on_device, tgt_d, seed_d), reps)
    got = [t.cpu().numpy() for t in native_mesh.locate(on_device, tgt_d, seed_d)]
    want, row["host_walk_s"] = wall(lambda: interp.locate_walk_host(src_xyz, mesh["tri"], mesh["nbr"], mesh["flag"], tgt_xyz, seed))
    row["kernel_equals_host_walk"] = bool(all(np.array_equal(g, w) for g, w in zip(got, want)))
    row["status_counts"] = [int(n) for n in np.bincount(got[2], minlength=4)]
    row["moves"] = dict(mean=float(got[3].mean()), max=int(got[3].max()))
    row["share_decided_by_host"] = float((got[2] == native_mesh.UNDECIDED).mean())
    row["host_walk_over_kernel"] = row["host_walk_s"] / (row["kernel"]["median_ms"] * 1e-3)

    kwargs = {} if max_edge_km is None else dict(max_edge_km=max_edge_km, outside="nearest")
    interp.linear_triangulated(src, tgt, device=True, **kwargs)  # warm: library load, allocator
    built, row["device_call_s"] = wall(lambda: interp.linear_triangulated(src, tgt, device=True, **kwargs))
    host, row["host_call_s"] = wall(lambda: interp.linear_triangulated(src, tgt, device=False, **kwargs))
    row["device_equals_host_bit_for_bit"] = bool(all(np.array_equal(host[k], built[k]) and host[k].dtype == built[k].dtype for k in host))
    return row


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "linear_unstructured_bench.json"))
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--cases", nargs="*", default=list(CASES))
    args = parser.parse_args()
    assert torch.cuda.is_available() and args.reps >= 20
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    result = dict(device=torch.cuda.get_device_name(dev), cases=[])
    for name in args.cases:
        row = run(name, dev, args.reps)
        result["cases"].append(row)
        print(json.dumps(row), flush=True)
        with open(args.json, "w") as f:  # after every case: a later case that runs out of time leaves the earlier ones
            json.dump(result, f, indent=1)
            f.write("\n")
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
