"""Interpolation on a coordinate field on the device: ``atx_coord_interpolate`` equals the numpy loop of include/atx_coord.h
(tests/coord_statement.py) bit for bit — NaN where the loop has NaN — lies within the header's bound of the exact statement, reports the
loop's ``bad`` points, gives the same bytes in every storage shape and writes nothing beyond a point's rows; then
``vertical.interpolate_on_coordinate`` where the variables overflow a workgroup's LDS, and the ``pl_to_hl`` filter end to end."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import coord_statement as cs
from anemoi_transform_amd import native_coord
from anemoi_transform_amd.fields import fieldlist_from_dicts
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.grids import lookup
from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack
from anemoi_transform_amd.vertical import interpolate_on_coordinate
from hybrid_column_common import CANARY, WIDTHS, allocate, assert_same_bits

pytestmark = pytest.mark.gpu

STORAGE = ("columns", "columns-pitch+1", "fields-pitch+3")  # the 16-byte routes where the shape allows, the scalar routes, the field-major kernel


def run_kernel(dev, T, shape, extras: bool, storage: str, outside: str):
    """The kernel on the shared case in one storage shape: ``(y [n_pts, n_var, n_tgt], bad)`` after asserting that everything of the
    output's allocation but a point's ``n_var x n_tgt`` rows (a row's ``n_pts`` points) still holds CANARY."""
    c, x, targets, offset, floor, _ = cs.case(np.dtype(T).name, shape, extras)
    n_pts, n_lev, n_var, n_tgt = shape
    columns = storage.startswith("columns")
    rows = dict(src=n_var * n_lev, coord=n_lev, out=n_var * n_tgt)
    values = dict(src=x.reshape(n_pts, -1), coord=c)
    stacks = {}
    for name, n in rows.items():
        stacks[name] = allocate(*((n_pts, n) if columns else (n, n_pts)), storage, T, dev, CANARY if name == "out" else float("nan"))
        if name != "out":
            stacks[name][:, : n if columns else n_pts] = torch.from_numpy(np.ascontiguousarray(values[name] if columns else values[name].T)).to(dev)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    bad = torch.full((n_pts + 16,), 7, dtype=torch.uint8, device=dev)
    native_coord.interpolate(stacks["src"], stacks["coord"], stacks["out"], up(targets), n_pts=n_pts, n_var=n_var, n_lev=n_lev, n_tgt=n_tgt,
                             src_pitch=stacks["src"].shape[1], coord_pitch=stacks["coord"].shape[1], out_pitch=stacks["out"].shape[1],
                             layout=COLUMNS if columns else FIELDS, offset=up(offset), floor=up(floor), bad=bad[:n_pts], outside=outside)
    torch.cuda.synchronize()
    width = rows["out"] if columns else n_pts
    host = stacks["out"]._base.cpu().numpy().copy()
    view = host[: stacks["out"].numel()].reshape(stacks["out"].shape)
    got = view[:, :width].copy()
    view[:, :width] = CANARY
    assert (host == CANARY).all() and (bad[n_pts:] == 7).all(), f"{shape} {storage}: written beyond a row"
    return (got if columns else np.ascontiguousarray(got.T)).reshape(n_pts, n_var, n_tgt), bad[:n_pts].cpu().numpy()


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "offset-floor"])
@pytest.mark.parametrize("shape", cs.SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("T", WIDTHS)
def test_the_kernel_is_the_statement_bit_for_bit_in_every_storage(dev, T, shape, extras):
    c, x, _, _, _, planted = cs.case(np.dtype(T).name, shape, extras)
    for outside in (cs.NEAREST, cs.MISSING):
        want, want_bad, interior = cs.reference(np.dtype(T).name, shape, extras, outside)
        first = None
        for storage in STORAGE:
            got, bad = run_kernel(dev, T, shape, extras, storage, outside)
            assert_same_bits(got, want, f"{shape} {storage} {outside}", "(point, variable, target)")
            assert np.array_equal(bad, want_bad) and sorted(np.flatnonzero(bad)) == sorted(planted), f"{shape} {storage}: bad differs from the statement's"
            first = got if first is None else first
            assert got.tobytes() == first.tobytes(), f"{shape} {outside}: {storage} differs from {STORAGE[0]}"
        worst = cs.worst_ulps(first, c, x, interior)
        print(f"coord kernel {np.dtype(T).name} {shape} extras={extras} {outside}: {worst:.4f} ulps from exact, bound {cs.bound(T):.9g}")
        assert worst <= cs.bound(T)


def test_variables_beyond_a_workgroups_lds_are_halved_with_the_same_bits(dev, monkeypatch):
    """80 float64 variables of 128 levels are 80 KiB a point: the column kernel refuses them, ``interpolate_on_coordinate`` launches two
    halves into the one result, and every variable has the bits of its own single-variable launch."""
    n_pts, n_lev, n_var = 40, 128, 80
    rng = np.random.default_rng(5)
    c = np.cumsum(rng.uniform(0.5, 2.0, (n_pts, n_lev)), axis=1)
    c[::3] = c[::3, ::-1]
    c[7, 60] = c[7, 59]
    x = rng.standard_normal((n_pts, n_var, n_lev))
    targets = [50.0, 1.0e4, 3.25, 77.125]
    stack, coord = Stack.from_fields(list(x.reshape(n_pts, -1).T), dev=dev), Stack.from_fields(list(c.T), dev=dev)
    launches, real = [], native_coord.interpolate

    def counted(*a, **k):
        launches.append(k["n_var"])
        return real(*a, **k)

    monkeypatch.setattr(native_coord, "interpolate", counted)
    out, bad = interpolate_on_coordinate(stack, coord, targets, n_var=n_var, outside="missing")
    assert launches == [80, 40, 40] and bad.cpu().tolist() == [int(p == 7) for p in range(n_pts)]
    got = out.numpy().reshape(n_var, len(targets), n_pts)
    for v in range(n_var):
        single, _ = interpolate_on_coordinate(Stack(stack.data[:, v * n_lev:(v + 1) * n_lev], n_pts, n_lev, COLUMNS), coord, targets, outside="missing")
        assert single.numpy().tobytes() == got[v].tobytes(), v
    want = cs.statement(c, x, np.array(targets), outside=cs.MISSING)[0]
    assert_same_bits(np.ascontiguousarray(got.transpose(2, 0, 1)), want, "halved launches", "(point, variable, target)")


# ---- the filter, end to end --------------------------------------------------------------------------------------------------------------
LEVELS_HPA = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
DATES, PARAMS = (20260101, 20260102), ("u", "v", "t")


def small_world(dtype):
    grid = lookup([10.0, 10.0])  # 684 points: more than one workgroup in either layout
    lat, lon = np.asarray(grid["latitudes"], dtype=np.float64), np.asarray(grid["longitudes"], dtype=np.float64)
    n, rng, specs, truth = len(lat), np.random.default_rng(31), [], {}
    for date in DATES:
        common = dict(latitudes=lat, longitudes=lon, date=date, time=0, step=0)
        zs = rng.uniform(-300.0, 20000.0, n).astype(dtype)
        z = (zs.astype(np.float64)[:, None] - 400.0 + np.cumsum(rng.uniform(800.0, 30000.0, (n, 13)), axis=1)[:, ::-1]).astype(dtype)  # falls as the pressure grows
        z[11, 4] = np.nan
        columns = {p: (20.0 * rng.standard_normal((n, 13))).astype(dtype) for p in PARAMS}
        specs.append(dict(values=zs, param="z", levtype="sfc", **common))
        for k in rng.permutation(13):  # the levels in no order
            for param in ("v", "z", "t", "u"):
                specs.append(dict(values=(z if param == "z" else columns[param])[:, k].copy(), param=param, levtype="pl", levelist=LEVELS_HPA[k], **common))
        truth[date] = (z, np.stack([columns[p] for p in ("v", "t", "u")], axis=1), zs)
    return fieldlist_from_dicts(specs, mars=True), truth


@pytest.mark.parametrize("reference,levels", [("ground", [10, 100, 250.5, 3000]), ("sea", [-50, 100, 250.5, 3000])])
@pytest.mark.parametrize("T", WIDTHS)
def test_pl_to_hl_end_to_end(dev, monkeypatch, caplog, T, reference, levels):
    data, truth = small_world(T)
    f = create_filter_by_name("pl_to_hl", levels=levels, reference=reference)
    launches, real = [], native_coord.interpolate
    monkeypatch.setattr(native_coord, "interpolate", lambda *a, **k: (launches.append((k["n_var"], k["n_lev"], k["n_tgt"])), real(*a, **k))[1])
    with caplog.at_level("WARNING"):
        result = list(f.forward(data))
    assert launches == [(3, 13, len(levels))] * len(DATES)  # ONE launch per group
    assert sum("not strictly monotone at 2 points of 2 groups" in r.getMessage() for r in caplog.records) == 1
    kept = list(data)
    assert all(a is b for a, b in zip(result, kept)) and len(result) == len(kept) + len(DATES) * 3 * len(levels)  # every input passes through
    new = result[len(kept):]
    assert [(g.metadata("date"), g.metadata("param"), g.metadata("levtype"), g.metadata("levelist")) for g in new] == [
        (date, param, "hl", level) for date in DATES for param in ("v", "t", "u") for level in levels]  # first seen first
    assert len({id(g.stack_ref()[0]) for g in new}) == len(DATES) and all(g.stack_ref()[0].data.is_cuda for g in new)  # levels of one resident stack
    assert all(g.stack_ref()[0].dtype == (torch.float32 if T is np.float32 else torch.float64) for g in new)
    targets = np.array(levels, dtype=np.float64) * np.float64(9.80665)
    for i, date in enumerate(DATES):
        z, x, zs = truth[date]
        got = np.stack([g.to_numpy(flatten=True) for g in new[i * 3 * len(levels):(i + 1) * 3 * len(levels)]], axis=1).reshape(-1, 3, len(levels))
        want, bad, _ = cs.statement(z, x, targets, **{"offset" if reference == "ground" else "floor": zs})
        assert bad.sum() == 1 and got.dtype == T
        assert_same_bits(got, want, f"pl_to_hl {reference} {date}", "(point, variable, target)")
