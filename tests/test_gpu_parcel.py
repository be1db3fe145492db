"""The parcel ascent on the device: ``atx_parcel_columns`` against the statement of include/atx_parcel.h (tests/parcel_statement.py) — NaN
exactly where the numpy loop has NaN, the same bytes in every storage shape, nothing written beyond a point's rows, ``pstart`` bit for
bit, and every finite value within twice numpy's own pinned error plus 2 ulps of the statement in 240-bit arithmetic; then the
``parcel_ascent`` filter end to end.

Every further point of a case is held to the numpy loop itself."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import parcel_statement as st
from anemoi_transform_amd import native_parcel
from anemoi_transform_amd.fields import fieldlist_from_dicts
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.grids import lookup
from anemoi_transform_amd.stack import COLUMNS, FIELDS
from hybrid_column_common import CANARY, WIDTHS, allocate

pytestmark = pytest.mark.gpu

STORAGE = ("columns", "columns-pitch+1", "fields-pitch+3")  # the 16-byte routes where the shape allows, the scalar routes, the field-major kernel


def run_kernel(dev, T, c: dict, parcel: str, storage: str) -> np.ndarray:
    """The kernel on a case in one storage shape: ``y [n_pts, 5]`` after asserting that everything of the output's allocation but a
    point's five rows (a row's ``n_pts`` points) still holds CANARY."""
    n_pts, n_lev = c["t"].shape
    columns = storage.startswith("columns")
    stacks = []
    for x in (c["t"], c["q"]):
        s = allocate(*((n_pts, n_lev) if columns else (n_lev, n_pts)), storage, T, dev, float("nan"))
        s[:, : n_lev if columns else n_pts] = torch.from_numpy(np.ascontiguousarray(x if columns else x.T)).to(dev)
        stacks.append(s)
    out = allocate(*((n_pts, 5) if columns else (5, n_pts)), storage, T, dev, CANARY)
    up = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    native_parcel.columns(*stacks, torch.from_numpy(c["sp"]).to(dev), out, n_pts=n_pts, n_lev=n_lev, t_pitch=stacks[0].shape[1], q_pitch=stacks[1].shape[1],
                          out_pitch=out.shape[1], layout=COLUMNS if columns else FIELDS, A=up(c["A"]), B=up(c["B"]), levels_pa=up(c["P"]), parcel=parcel,
                          depth_pa=st.DEPTH, top_pa=st.TOP)
    torch.cuda.synchronize()
    width = 5 if columns else n_pts
    host = out._base.cpu().numpy().copy()
    view = host[: out.numel()].reshape(out.shape)
    got = view[:, :width].copy()
    view[:, :width] = CANARY
    assert (host == CANARY).all(), f"{storage}: written beyond a row"
    return got if columns else np.ascontiguousarray(got.T)


def check(got: np.ndarray, dtype: str, n_lev: int, n_pts: int, mode: str, parcel: str, what: str) -> None:
    """``got [n_pts, 5]`` in the case's type against the statement: the first points against 240-bit arithmetic, EVERY point against the
    numpy loop within 1e-10 of its unit's size (S, |y|) plus one ulp of the type — kernel and numpy are each within some 10^3 float64
    ulps, 10^-13, of exact (the host test's cap), so a thousand times that separates rounding from a defect."""
    want, exact, unit, _, S = st.reference(dtype, n_lev, n_pts, mode, parcel)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    assert got[:, 4].tobytes() == want[:, 4].astype(got.dtype).tobytes(), f"{what}: pstart is a copy"
    size = np.where(np.arange(5)[None, :] < 2, S[:, None], np.abs(want))
    with np.errstate(invalid="ignore"):
        far = np.abs(got.astype(np.float64) - want) > 1e-10 * size + np.spacing(size.astype(got.dtype)).astype(np.float64)
    assert not far.any(), f"{what}: (point, output) {np.argwhere(far)[:5].tolist()} lie far from the numpy loop"
    bound, numpy_worst = st.budget(dtype, n_lev, n_pts, mode, parcel)
    e = st.errors(got[: len(exact)], exact, unit)
    for o, name in enumerate(st.OUTPUTS):
        worst = float(np.nanmax(e[:, o])) if np.isfinite(e[:, o]).any() else 0.0
        print(f"{what} {name}: kernel {worst:.4f} ulps from exact, numpy float64 {numpy_worst[o]:.4f}, bound {bound[o]:.4f}")
        assert worst <= bound[o], f"{what} {name}: {worst:.4f} ulps from exact > {bound[o]:.4f} (numpy's float64 arithmetic: {numpy_worst[o]:.4f})"


@pytest.mark.parametrize("parcel", [st.LOWEST, st.MOST_UNSTABLE])
@pytest.mark.parametrize("mode", [st.HYBRID, st.PRESSURE])
@pytest.mark.parametrize("n_lev", st.N_LEVS)
@pytest.mark.parametrize("T", WIDTHS)
def test_the_kernel_is_the_statement_in_every_storage(dev, T, n_lev, mode, parcel):
    dtype = np.dtype(T).name
    tile = native_parcel.tile_points(n_lev, torch.float32 if T is np.float32 else torch.float64, pressure_levels=mode == st.PRESSURE, parcel=parcel)
    assert tile > 0
    for n_pts in (tile + 1, 1):  # the last tile is partial; a single point
        c, first = st.case(dtype, n_lev, n_pts, mode), None
        for storage in STORAGE:
            got = run_kernel(dev, T, c, parcel, storage)
            first = got if first is None else first
            assert got.tobytes() == first.tobytes(), f"{n_lev} x {n_pts} {mode} {parcel}: {storage} differs from {STORAGE[0]}"
        check(first, dtype, n_lev, n_pts, mode, parcel, f"{dtype} {n_lev} x {n_pts} {mode} {parcel}")


# ---- the filter, end to end --------------------------------------------------------------------------------------------------------------
DATES = (20260101, 20260102)
NAMES = {"cape": "cape", "cin": "mucin", "plcl": "plcl", "pstart": "pstart"}


@pytest.mark.parametrize("levtype", ["ml", "pl"])
@pytest.mark.parametrize("T", WIDTHS)
def test_parcel_ascent_end_to_end(dev, monkeypatch, T, levtype):
    grid = lookup([10.0, 10.0])  # 684 points: more than one workgroup in either layout
    lat, lon = np.asarray(grid["latitudes"], dtype=np.float64), np.asarray(grid["longitudes"], dtype=np.float64)
    n, n_lev, dtype, mode = len(lat), 9, np.dtype(T).name, st.HYBRID if levtype == "ml" else st.PRESSURE
    c = st.case(dtype, n_lev, n, mode)
    if levtype == "ml":
        levels, config = list(range(1, n_lev + 1)), dict(levtype="ml", model_level_AB=dict(A=list(c["A"]), B=list(c["B"])))
    else:
        levels, config = [float(v) / 100.0 for v in c["P"]], dict(levtype="pl")
    rng, specs = np.random.default_rng(5), []
    for date in DATES:
        common = dict(latitudes=lat, longitudes=lon, date=date, time=0, step=0)
        specs.append(dict(values=c["sp"], param="sp", levtype="sfc", **common))
        for k in rng.permutation(n_lev):  # the levels in no order
            for param in ("q", "t"):
                specs.append(dict(values=c[param][:, k].copy(), param=param, levtype=levtype, levelist=levels[k], **common))
    data = fieldlist_from_dicts(specs, mars=True)
    f = create_filter_by_name("parcel_ascent", outputs=NAMES, parcel="most-unstable", depth=st.DEPTH / 100.0, top=st.TOP / 100.0, **config)
    launches, real = [], native_parcel.columns
    monkeypatch.setattr(native_parcel, "columns", lambda *a, **k: (launches.append((k["n_pts"], k["n_lev"])), real(*a, **k))[1])
    result = list(f.forward(data))
    assert launches == [(n, n_lev)] * len(DATES)  # ONE launch per group
    kept = list(data)
    assert all(a is b for a, b in zip(result, kept)) and len(result) == len(kept) + len(DATES) * len(NAMES)  # every input passes through
    new = result[len(kept):]
    assert [(g.metadata("date"), g.metadata("param"), g.metadata("levtype")) for g in new] == [(date, name, "sfc") for date in DATES for name in NAMES.values()]
    assert len({id(g.stack_ref()[0]) for g in new}) == len(DATES) and all(g.stack_ref()[0].data.is_cuda for g in new)  # levels of one resident stack
    assert all(g.stack_ref()[0].dtype == (torch.float32 if T is np.float32 else torch.float64) for g in new)
    for i in range(len(DATES)):
        got = np.full((n, 5), np.nan, dtype=T)
        for g, name in zip(new[i * len(NAMES):(i + 1) * len(NAMES)], NAMES):
            got[:, st.OUTPUTS.index(name)] = g.to_numpy(flatten=True)
        want = st.reference(dtype, n_lev, n, mode, st.MOST_UNSTABLE)[0].astype(T)
        got[:, 3] = want[:, 3]  # (tlcl is not asked for)
        check(got, dtype, n_lev, n, mode, st.MOST_UNSTABLE, f"parcel_ascent {levtype} {DATES[i]}")
