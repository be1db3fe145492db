"""The parcel ascent at the shapes it is for: O1280 x 137 model levels and 0.25 degrees x 13 pressure levels, the lowest parcel, all five
outputs, float32 and float64.

    python tools/parcel_bench.py --json profiles/parcel_bench.json

Per shape and type, in ONE process, interleaved round by round (device events around every call, every series warmed first), on the same
buffers:
  - ``columns`` / ``columns_again``   ``vertical.lift_parcels`` on column stacks — the LDS-tile kernel, a lane per (point, level) — timed as
                                      TWO series in every round: the difference of their medians is the run-to-run spread;
  - ``fields``                        the same call on field-major stacks that are already there: one lane per point;
  - ``relayout_fields``               a column stack served through the field-major kernel: both stacks relaid, the call, the result
                                      relaid back — what ``PARCEL_COLUMNS_ROUTE = "fields"`` would cost a filter;
  - ``torch``                         the same statement with torch on the same device, float64, in chunks of ``TORCH_CHUNK`` points (its
                                      temporaries are ``[points, levels]`` each): every level solved by the 10 capped Newton steps and
                                      selected by masks, the sums by ``sum`` (not blocked);
  - ``copy``                          a plain device copy that reads and writes the ALGORITHMIC bytes — t, q and sp read, five rows
                                      written: the byte bound of any design, which this kernel is far from by construction.
Recorded: median / min / max per series, the kernel over the copy and over torch, whether the layouts give the same bits and how far
torch's cape is from the kernel's.  NOT measured here: kernel time apart from the launch (no profiler run), counters, more than one
device, the most unstable parcel, the phases apart, other tile sizes or Newton counts, shapes other than those named.  ``--small`` shrinks
the grids for a rehearsal; the committed record is the default.
"""

from __future__ import annotations

import argparse
import gc
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
from anemoi_transform_amd.grids import lookup  # noqa: E402
from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack  # noqa: E402
from anemoi_transform_amd.vertical import lift_parcels  # noqa: E402

PEAK = 8e12
SHAPES = [("o1280", 137, "ml"), ("0.25", 13, "pl")]  # (grid, levels, levtype)
PL_HPA = (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)
TOP_PA = 5000.0
TORCH_CHUNK = 1 << 19
RD, RV, LN1E5 = 287.0597, 461.5250, 11.512925464970229


def spread(ms: list) -> dict:
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=len(ms))


def timed(fn) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def run_series(series: dict, reps: int, warm: int) -> dict:
    names = list(series)
    for _ in range(warm):
        for name in names:
            series[name]()
            gc.collect()  # (between calls, outside every timed region)
    torch.cuda.synchronize()
    ms = {name: [] for name in names}
    for r in range(reps):
        for i in range(len(names)):  # a rotating order: no series always follows the same neighbour
            name = names[(i + r) % len(names)]
            ms[name].append(timed(series[name]))
            gc.collect()
    return {name: spread(v) for name, v in ms.items()}


def eta_table(n_lev: int):
    eta = np.arange(n_lev + 1, dtype=np.float64) / n_lev
    return 20000.0 * eta * (1.0 - eta), (np.maximum(eta - 0.3, 0.0) / 0.7) ** 2


def torch_chunk(t, q, sp, p):
    """include/atx_parcel.h with torch, the lowest parcel: ``t``, ``q``, ``p`` ``[n, n_lev]`` float64, ``sp [n]`` -> ``[n, 5]``."""
    eps, n_lev = RD / RV, t.shape[1]
    k = torch.arange(n_lev, device=t.device)[None, :]
    part = (p >= TOP_PA) & (p <= sp[:, None])
    kb = torch.where(part, k, -1).amax(dim=1, keepdim=True)
    at = lambda x: x.gather(1, kb.clamp(min=0))  # noqa: E731
    lnp, r_env = p.log(), q / (1.0 - q)
    H = lambda lnT, TL, r: (lnT + (0.2854 * (1.0 - 0.28 * r)) * (LN1E5 - lnp)) + ((3.376 / TL - 0.00254) * (1000.0 * r)) * (1.0 + 0.81 * r)  # noqa: E731
    Ts, rs, ps = at(t), at(r_env), at(p)
    e = ps * rs / (eps + rs)
    TL = 2840.0 / ((3.5 * Ts.log() - (e / 100.0).log()) - 4.805) + 55.0
    target = (Ts.log() + (0.2854 * (1.0 - 0.28 * rs)) * (LN1E5 - ps.log())) + ((3.376 / TL - 0.00254) * (1000.0 * rs)) * (1.0 + 0.81 * rs)
    pL = ps * (3.5 * (TL / Ts).log()).exp()
    Td = Ts * ((2.0 / 7.0) * (p / ps).log()).exp()
    lh = (p / 1222.42).log()
    cap = (32.19 * lh - 4780.84632) / (lh - 17.502)
    sat = lambda T: 611.21 * ((17.502 * (T - 273.16)) / (T - 32.19)).exp()  # noqa: E731
    T = Td.clone()
    for _ in range(10):
        es = sat(T)
        pe = p - es
        r = eps * es / pe
        dr = r * (p / pe) * (4217.45694 / (T - 32.19) ** 2)
        w = 1000.0 * r * (1.0 + 0.81 * r)
        dF = (1.0 / T - 0.079912 * dr * (LN1E5 - lnp)) - 3.376 / (T * T) * w + (3.376 / T - 0.00254) * 1000.0 * dr * (1.0 + 1.62 * r)
        T = torch.minimum(T - (H(T.log(), T, r) - target) / dF, cap)
    es = sat(T)
    moist = p < pL
    Tp, rp = torch.where(moist, T, Td), torch.where(moist, eps * es / (p - es), rs.expand_as(p))
    tv = lambda T_, r_: T_ * (1.0 + r_ / eps) / (1.0 + r_)  # noqa: E731
    b = torch.where(part & (k < kb), RD * (tv(Tp, rp) - tv(t, r_env)), torch.zeros_like(t))
    lo, hi, dl = b[:, 1:], b[:, :-1], lnp[:, 1:] - lnp[:, :-1]
    step = part[:, :-1] & (k[:, :-1] < kb)
    split = ((lo > 0) & (hi < 0)) | ((lo < 0) & (hi > 0))
    f = torch.where(split, lo / torch.where(split, lo - hi, torch.ones_like(lo)), torch.zeros_like(lo))
    a_lo, a_hi, area = lo * f * dl / 2.0, hi * (1.0 - f) * dl / 2.0, (lo + hi) / 2.0 * dl
    pos = torch.where(split, torch.where(lo > 0, a_lo, a_hi), area.clamp(min=0.0)) * step
    neg = torch.where(split, torch.where(lo > 0, a_hi, a_lo), area.clamp(max=0.0)) * step
    first = torch.where(pos > 0, k[:, :-1], -1).amax(dim=1, keepdim=True)
    below = (k[:, :-1] > first) | ((k[:, :-1] == first) & (lo < 0))
    cin = torch.where(first >= 0, (neg * below).sum(dim=1, keepdim=True), torch.full_like(Ts, float("nan")))
    out = torch.cat([pos.sum(dim=1, keepdim=True), cin, pL, TL, ps], dim=1)
    return torch.where(kb >= 0, out, torch.full_like(out, float("nan")))


def torch_statement(t, q, sp, A, B, P) -> torch.Tensor:
    out = []
    for i in range(0, t.shape[0], TORCH_CHUNK):
        s = sp[i:i + TORCH_CHUNK].double()
        if P is None:
            half = A[None, :] + B[None, :] * s[:, None]
            p = (half[:, :-1] + half[:, 1:]) / 2.0
        else:
            p = P[None, :].expand(s.numel(), -1)
        out.append(torch_chunk(t[i:i + TORCH_CHUNK].double(), q[i:i + TORCH_CHUNK].double(), s, p).to(t.dtype))
    return torch.cat(out)


def measure(n_pts: int, n_lev: int, levtype: str, tdt, dev, reps: int, warm: int) -> dict:
    itemsize = 4 if tdt == torch.float32 else 8
    gen = torch.Generator(device=dev).manual_seed(itemsize * 100 + n_lev)
    sp = (96000.0 + 7000.0 * torch.rand(n_pts, device=dev, generator=gen, dtype=torch.float64)).to(tdt)
    if levtype == "ml":
        A, B = (torch.tensor(c, device=dev) for c in eta_table(n_lev))
        half = A[None, :] + B[None, :] * sp[:, None].double()
        p, table, P = (half[:, :-1] + half[:, 1:]) / 2.0, dict(A=A, B=B), None
    else:
        A = B = None
        P = torch.tensor(PL_HPA, dtype=torch.float64, device=dev) * 100.0
        p, table = P[None, :].expand(n_pts, -1), dict(levels_pa=[100.0 * v for v in PL_HPA])  # (a host list, as the filter passes it)
    # a conditionally unstable column: 300 K at the ground, d ln T / d ln p = 0.19 + noise, 80 % humidity falling with height
    x = p / sp[:, None].double()
    t64 = torch.clamp((298.0 + 6.0 * torch.rand((n_pts, 1), device=dev, generator=gen, dtype=torch.float64)) * x ** 0.19, min=205.0)
    e = 0.8 * x.clamp(0.02, 1.0) ** 1.5 * 611.21 * torch.exp(17.502 * (t64 - 273.16) / (t64 - 32.19))
    t, q = Stack.empty(n_pts, n_lev, tdt, dev, COLUMNS, zero=True), Stack.empty(n_pts, n_lev, tdt, dev, COLUMNS, zero=True)
    t.data[:, :n_lev], q.data[:, :n_lev] = t64.to(tdt), (0.622 * e / (p - 0.378 * e)).to(tdt)
    del x, t64, e, p
    tf, qf = t.to_layout(FIELDS), q.to_layout(FIELDS)
    alg = (2 * n_lev + 1 + 5) * n_pts * itemsize
    half_a, half_b = torch.empty(alg // 2, dtype=torch.uint8, device=dev), torch.empty(alg // 2, dtype=torch.uint8, device=dev)
    call = lambda a, b: lift_parcels(a, b, sp, top_pa=TOP_PA, **table)  # noqa: E731
    tt, qt = t.data[:, :n_lev], q.data[:, :n_lev]
    series = {
        "columns": lambda: call(t, q),
        "columns_again": lambda: call(t, q),
        "fields": lambda: call(tf, qf),
        "relayout_fields": lambda: call(t.to_layout(FIELDS), q.to_layout(FIELDS)).to_layout(COLUMNS),
        "torch": lambda: torch_statement(tt, qt, sp, A, B, P),
        "copy": lambda: half_b.copy_(half_a),
    }
    got = run_series(series, reps, warm)
    y, yf, yt = call(t, q).data[:, :5], call(tf, qf).to_layout(COLUMNS).data[:, :5], torch_statement(tt, qt, sp, A, B, P)
    bits = torch.int32 if itemsize == 4 else torch.int64
    a, b = got["columns"]["median_ms"], got["columns_again"]["median_ms"]
    kernel = 0.5 * (a + b)
    cape, cape_t = y[:, 0].double(), yt[:, 0].double()
    return dict(series=got, algorithmic_bytes=alg, columns_run_to_run_spread=abs(a - b) / min(a, b), columns_over_copy=kernel / got["copy"]["median_ms"],
                fields_over_copy=got["fields"]["median_ms"] / got["copy"]["median_ms"], torch_over_columns=got["torch"]["median_ms"] / kernel,
                fields_over_columns=got["fields"]["median_ms"] / kernel, relayout_fields_over_columns=got["relayout_fields"]["median_ms"] / kernel,
                copy_fraction_of_peak=alg / (got["copy"]["median_ms"] * 1e-3) / PEAK,
                layouts_give_the_same_bits=bool(torch.equal(y.contiguous().view(bits), yf.contiguous().view(bits))),
                torch_cape_max_relative_difference=float(((cape_t - cape).abs() / cape.abs().clamp(min=1.0)).max()),
                points_with_cape=int((cape > 0).sum()), mean_cape=float(cape.mean()))


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--json", default=os.path.join(ROOT, "profiles", "parcel_bench.json"))
    parser.add_argument("--small", action="store_true", help="10 degree and o32 grids: a rehearsal of the script, not a measurement")
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--warm", type=int, default=2)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing here falls back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    grids = {"0.25": "10.0" if args.small else "0.25", "o1280": "o32" if args.small else "o1280"}
    result = dict(device=torch.cuda.get_device_name(dev), peak_bytes_per_s=PEAK, reps=args.reps, warm=args.warm, parcel="lowest", top_pa=TOP_PA, grids=grids,
                  not_measured="kernel time apart from the launch, counters, more than one device, the most unstable parcel, the phases apart, "
                               "other tile sizes or Newton counts, other shapes", shapes={})
    for grid, n_lev, levtype in SHAPES:
        name = grids[grid]
        n_pts = len(lookup([float(name), float(name)] if name[0].isdigit() else name)["latitudes"])
        for tdt, tag in ((torch.float32, "float32"), (torch.float64, "float64")):
            key = f"{name}_x_{n_lev}_{levtype}_{tag}"
            result["shapes"][key] = dict(n_pts=n_pts, **measure(n_pts, n_lev, levtype, tdt, dev, args.reps, args.warm))
            print(key, json.dumps(result["shapes"][key]), flush=True)
            torch.cuda.empty_cache()
            with open(args.json, "w") as f:  # after every shape: a run cut short leaves what it measured
                json.dump(result, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
