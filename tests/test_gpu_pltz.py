"""``atx_pltz_interpolate`` on the device against the restatement of include/atx_pltz.h (tests/pltz_statement.py): NaN exactly where the
restatement has NaN, msl == p_g bit for bit where |zs| < 0.001, every other value within the class's bound of the exact statement, the
storage shapes byte-identical to each other — then the ``ml_to_pl_tz`` filter end to end and against the existing two-filter route.

The rule (``levels_restatement.log_budget``): float64 within 2 x numpy's pinned worst error of the class + 2 ulps
(tests/test_pltz_host.py::NUMPY_WORST_PLTZ); float32 0.5 ulp + that bound x 2^-29.  Units: the ulp of |y| for t and msl, of
max(|zs|, max_k |c[k]|) of the point for z.  The kernel's worst per class is printed and written as JSON to the file that
``ATX_PLTZ_ULPS_JSON`` names, if it is set (profiles/pltz_ulps.json).
"""

from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import geopotential_restatement as gr
import pltz_statement as ps
from anemoi_transform_amd import native_pltz
from anemoi_transform_amd.fields import fieldlist_from_dicts
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.grids import lookup
from anemoi_transform_amd.stack import COLUMNS, FIELDS
from hybrid_column_common import CANARY, WIDTHS, allocate
from test_pltz_host import NUMPY_WORST_PLTZ

pytestmark = pytest.mark.gpu
STORAGE = ("columns", "columns-pitch+1", "fields-pitch+3")
REPORT: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT and os.environ.get("ATX_PLTZ_ULPS_JSON"):
        with open(os.environ["ATX_PLTZ_ULPS_JSON"], "w") as f:
            json.dump(dict(unit="ulps of |y| (t, msl) or of max(|zs|, max |c[k]|) (z) in the stack's type; [kernel, bound]", kernel=REPORT), f, indent=1)
            f.write("\n")


def run_kernel(dev, name: str, storage: str, coordinate: str) -> np.ndarray:
    """``[n_pts, 2 n_tgt + 1]`` of the case in one storage shape, after asserting that nothing else of out's allocation was written."""
    geo, targets = ps.CASES[name]
    n_pts, n_lev, rows, columns = geo.n_pts, geo.n_lev, 2 * len(targets) + 1, not storage.startswith("fields")
    stacks = {}
    for key, n in (("t", n_lev), ("q", n_lev), ("out", rows)):
        stacks[key] = allocate(*((n_pts, n) if columns else (n, n_pts)), storage, geo.T, dev, CANARY if key == "out" else float("nan"))
        if key != "out":
            values = torch.from_numpy(getattr(geo, key)).to(dev)
            stacks[key][:, : (n if columns else n_pts)] = values if columns else values.T
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    native_pltz.interpolate(stacks["t"], stacks["q"], up(geo.sp), up(geo.zs), stacks["out"], up(geo.A), up(geo.B), up(targets), n_pts=n_pts, n_lev=n_lev,
                            n_tgt=len(targets), t_pitch=stacks["t"].shape[1], q_pitch=stacks["q"].shape[1], out_pitch=stacks["out"].shape[1],
                            layout=COLUMNS if columns else FIELDS, coordinate=coordinate, msl=True)
    torch.cuda.synchronize()
    host = stacks["out"].cpu().numpy()
    width = rows if columns else n_pts
    assert (host[:, width:] == CANARY).all(), f"{name} {storage}: written beyond a row"
    return np.ascontiguousarray(host[:, :width] if columns else host[:, :width].T)


def assert_under_the_rule(got: np.ndarray, name: str, coordinate: str, pinned, report_key=None) -> None:
    geo, targets = ps.CASES[name]
    log = coordinate == ps.LOG
    want, exact, _, infos = ps.reference(name, log)
    assert got.dtype == geo.T and np.array_equal(np.isnan(got), np.isnan(want)), f"{name}: NaN differ at {np.argwhere(np.isnan(got) != np.isnan(want))[:5].tolist()}"
    small = np.array([abs(float(geo.zs[p])) < 0.001 for p in range(geo.n_pts)])
    assert small.any() and np.array_equal(got[small, -1], np.array([info["pg"] for info in infos])[small].astype(geo.T))  # msl == p_g, bit for bit
    worst = ps.worst_errors(got, name, log)
    bounds = {key: ps.bound(geo.T, value) for key, value in zip(("t", "z", "msl"), pinned)}
    if report_key:
        REPORT[report_key] = {key: (worst[key], bounds[key]) for key in bounds}
    print(name, coordinate, worst, bounds)
    for key in bounds:
        assert worst[key] <= bounds[key], f"{name} {coordinate}: {key} is {worst[key]:.4f} ulps from exact > {bounds[key]:.6g}"


@pytest.mark.parametrize("shape", ps.SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("coordinate", [ps.LINEAR, ps.LOG])
@pytest.mark.parametrize("T", WIDTHS)
def test_the_kernel_is_within_its_budget_of_the_exact_statement(dev, T, coordinate, shape):
    name = ps.make_case(T, *shape)
    first = run_kernel(dev, name, STORAGE[0], coordinate)
    for storage in STORAGE[1:]:
        assert run_kernel(dev, name, storage, coordinate).tobytes() == first.tobytes(), f"{name} {coordinate}: {storage} differs from {STORAGE[0]}"
    assert_under_the_rule(first, name, coordinate, NUMPY_WORST_PLTZ[(shape[1], coordinate)], f"{name} {coordinate}")


# ---- the filter, end to end --------------------------------------------------------------------------------------------------------------
N_LEV, DATES = 17, (20260101, 20260102)
LEVELS = list(ps.WORLD_LEVELS["filter"])  # hPa, in no order


def small_world(dtype, which):
    """A 10 degree grid (684 points), two dates, each a case of ``pltz_statement.world_case`` (the host test holds their margins) with
    the fields' levels in no order."""
    grid = lookup([10.0, 10.0])
    lat, lon = np.asarray(grid["latitudes"], dtype=np.float64), np.asarray(grid["longitudes"], dtype=np.float64)
    specs, names = [], {}
    rng = np.random.default_rng(31)
    for seed, date in zip(ps.WORLD_SEEDS, DATES):
        name = names[date] = ps.world_case(dtype, which, seed)
        geo = ps.CASES[name][0]
        assert (geo.n_pts, geo.n_lev) == (len(lat), N_LEV)
        common = dict(latitudes=lat, longitudes=lon, date=date, time=0, step=0)
        specs.append(dict(values=geo.zs, param="z", levtype="ml", levelist=1, **common))  # as MARS keeps it
        specs.append(dict(values=geo.sp, param="sp", levtype="sfc", **common))
        for level in rng.permutation(N_LEV) + 1:
            for param, column in (("q", geo.q), ("t", geo.t), ("u", geo.q)):
                specs.append(dict(values=column[:, level - 1].copy(), param=param, levtype="ml", levelist=int(level), **common))
    return fieldlist_from_dicts(specs, mars=True), names, dict(A=geo.A.tolist(), B=geo.B.tolist())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_filter_end_to_end(dev, monkeypatch, dtype):
    data, names, AB = small_world(dtype, "filter")
    f = create_filter_by_name("ml_to_pl_tz", levels=LEVELS, model_level_AB=AB, interpolation="log")
    launches, real = [], native_pltz.interpolate
    monkeypatch.setattr(native_pltz, "interpolate", lambda *a, **k: (launches.append((k["n_lev"], k["n_tgt"])), real(*a, **k))[1])
    result, kept = list(f.forward(data)), list(data)
    assert launches == [(N_LEV, len(LEVELS))] * len(DATES)  # ONE launch per group
    per_date = 2 * len(LEVELS) + 1
    assert all(a is b for a, b in zip(result, kept)) and len(result) == len(kept) + len(DATES) * per_date  # every input passes through
    new = result[len(kept):]
    assert [(g.metadata("date"), g.metadata("param"), g.metadata("levtype"), g.metadata("levelist", default=None)) for g in new] == [
        key for date in DATES for key in [(date, p, "pl", v) for p in ("t", "z") for v in LEVELS] + [(date, "msl", "sfc", None)]]
    assert len({id(g.stack_ref()[0]) for g in new}) == len(DATES)  # levels of one resident stack per group
    assert all(g.stack_ref()[0].data.is_cuda and g.stack_ref()[0].dtype == (torch.float32 if dtype is np.float32 else torch.float64) for g in new)
    for i, date in enumerate(DATES):
        got = np.stack([g.to_numpy(flatten=True) for g in new[i * per_date:(i + 1) * per_date]], axis=1)
        worst = ps.numpy_worst(names[date], True)  # numpy's worst ON THIS CASE, measured here on the CPU
        assert_under_the_rule(got, names[date], ps.LOG, (worst["t"], worst["z"], worst["msl"]))


def test_interior_targets_agree_with_the_two_filter_route(dev):
    """At targets that are interior for every point: t is ``ml_to_pl``'s bit for bit in the linear coordinate (no library function in it);
    z agrees with ``geopotential_on_model_levels | ml_to_pl`` within the sum of the two routes' bounds — this kernel's for z (in ulps of
    max(|zs|, max |c[k]|)) and the geopotential kernel's, whose unit U[k] <= |zs| + |c[k] - zs| is below four of those ulps."""
    levels = list(ps.WORLD_LEVELS["interior"])
    data, names, AB = small_world(np.float64, "interior")
    data = [g for g in data if g.metadata("param") != "u"]
    mine = [g for g in create_filter_by_name("ml_to_pl_tz", levels=levels, model_level_AB=AB, msl=False).forward(data) if g.metadata("levtype") == "pl"]
    route = create_filter_by_name("geopotential_on_model_levels", model_level_AB=AB) | create_filter_by_name("ml_to_pl", levels=levels, model_level_AB=AB, params=["t", "z"])
    theirs = {(g.metadata("date"), g.metadata("param"), g.metadata("levelist")): g.to_numpy(flatten=True) for g in route.forward(data) if g.metadata("levtype") == "pl"}
    assert len(mine) == len(theirs) == 2 * 2 * len(levels)
    for g in mine:
        date, param = g.metadata("date"), g.metadata("param")
        geo = ps.CASES[names[date]][0]
        keep = np.isfinite(geo.zs)  # (a NaN zs makes every output of this filter NaN; ml_to_pl's t does not read it)
        a, b = g.to_numpy(flatten=True)[keep], theirs[(date, param, g.metadata("levelist"))][keep]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.isfinite(a).sum() > 500
        if param == "t":
            assert np.array_equal(a, b, equal_nan=True)
            continue
        c = gr.reference(geo, rounded=False)
        unit = np.spacing(np.nan_to_num(np.abs(np.column_stack([c, geo.zs]))).max(axis=1))[keep]
        ulps = ps.bound(np.float64, ps.numpy_worst(names[date], False)["z"]) + 4.0 * gr.bound(geo, gr.numpy_worst(geo))
        finite = ~np.isnan(a)
        assert (np.abs(a - b)[finite] <= ulps * unit[finite]).all(), (date, float(np.nanmax(np.abs(a - b) / unit)), ulps)
