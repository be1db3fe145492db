"""Geopotential on model levels on the device: ``atx_geopotential_on_model_levels`` against the restatement of include/atx_geopotential.h
(tests/geopotential_restatement.py) — NaN and infinities exactly where the restatement has them, every finite value within the class's
bound of the exact statement (float64: twice numpy's PINNED worst error of the class plus SLACK, tests/test_geopotential_host.py::
NUMPY_WORST_GEOPOTENTIAL; float32: one rounding and 2^-29 of that), model level 0 alone — no logarithm — bit for bit, every storage shape
byte-identical to the others — then ``vertical.geopotential_on_model_levels``, the filter, and the filter into ``ml_to_pl``.

Worst distance from exact measured on an MI355X, in ulps of U (profiles/geopotential_ulps.json): float64 2147.75 for the whole 137 levels
(numpy's own arithmetic: 2147.75, bound 4297.5), 13173.64 for the lowest 137 of 145 without zs (bound 26349.28), 850.05 / 2474.12 for 60
levels, 2.92 / 25.69 for three, 2.74 (numpy 2.44, bound 6.88) / 29.87 for two, 24.43 for one level of a longer table; float32 at most
0.49999 (bound 0.5 + 2^-29 of the float64 ceiling) — the same bytes in every storage shape.  The test prints the figures of its run and
writes them as JSON to the file that ``ATX_GEOPOTENTIAL_ULPS_JSON`` names, if it is set.
"""

from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import geopotential_restatement as gr
import levels_restatement as lr
from anemoi_transform_amd import native_geopotential
from anemoi_transform_amd.fields import FieldList, fieldlist_from_dicts, new_field_from_stack
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.grids import lookup
from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack
from anemoi_transform_amd.vertical import geopotential_on_model_levels
from hybrid_column_common import CANARY, COLUMN_STORAGE, FIELD_STORAGE, WIDTHS, allocate
from test_geopotential_host import NUMPY_WORST_GEOPOTENTIAL

pytestmark = pytest.mark.gpu

# the storages it shares with the levels test, and between them t on the 16-byte route with q on the scalar one
STORAGE = COLUMN_STORAGE + ("columns-t-aligned-q-pitch+1",) + FIELD_STORAGE


def run_kernel(dev, case: gr.GeoCase, storage: str, n_pts: int) -> np.ndarray:
    """The kernel on the case's columns repeated cyclically to ``n_pts`` points, in one storage shape: ``[n_pts, n_lev]``.  Asserts that
    nothing is written outside a point's ``n_lev`` rows (or a row's ``n_pts`` points) and that t, q, sp and zs are left as they were."""
    n_lev = case.n_lev
    columns = storage.startswith("columns")
    layout = COLUMNS if columns else FIELDS
    mixed = storage == "columns-t-aligned-q-pitch+1"
    shape = (n_pts, n_lev) if columns else (n_lev, n_pts)
    t = allocate(*shape, "columns" if mixed else storage, case.T, dev, float("nan"))
    q = allocate(*shape, "columns-pitch+1" if mixed else storage, case.T, dev, float("nan"))
    out = allocate(*shape, "columns" if mixed else storage, case.T, dev, CANARY)
    for dst, values in ((t, gr.expand(case.t, n_pts)), (q, gr.expand(case.q, n_pts))):
        if columns:
            dst[:, :n_lev] = torch.from_numpy(values).to(dev)
        else:
            dst[:, :n_pts] = torch.from_numpy(np.ascontiguousarray(values.T)).to(dev)
    sp = torch.from_numpy(gr.expand(case.sp, n_pts)).to(dev)
    zs = None if case.zs is None else torch.from_numpy(gr.expand(case.zs, n_pts)).to(dev)
    before = [x.clone() for x in (t, q, sp)] + ([] if zs is None else [zs.clone()])
    f64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    native_geopotential.geopotential(t, q, sp, zs, f64(case.A), f64(case.B), out, n_pts=n_pts, n_lev=n_lev, t_pitch=t.stride(0), q_pitch=q.stride(0),
                               out_pitch=out.stride(0), layout=layout)
    torch.cuda.synchronize()
    bits = torch.int32 if case.T is np.float32 else torch.int64
    for name, now, was in zip(("t", "q", "sp", "zs"), [t, q, sp] + ([] if zs is None else [zs]), before):
        assert torch.equal(now.view(bits), was.view(bits)), f"{case.name} {storage}: {name} was modified"
    host = out.cpu().numpy()
    if columns:
        assert (host[:, n_lev:] == CANARY).all(), f"{case.name} {storage}: written beyond a point's {n_lev} rows"
        return host[:, :n_lev].copy()
    assert (host[:, n_pts:] == CANARY).all(), f"{case.name} {storage}: written beyond the {n_pts} points of a row"
    return np.ascontiguousarray(host[:, :n_pts].T)


def expanded(case: gr.GeoCase, n_pts: int) -> gr.GeoCase:
    """The case at ``n_pts`` points: what the comparison sees.  Its references are those of the 48 columns, repeated — never recomputed."""
    big = gr.GeoCase(f"{case.name}-x{n_pts}", case.T, case.A, case.B, gr.expand(case.sp, n_pts), gr.expand(case.zs, n_pts), gr.expand(case.t, n_pts),
                     gr.expand(case.q, n_pts))
    for rounded in (True, False):
        gr._REFERENCES.setdefault((big.name, rounded), gr.expand(gr.reference(case, rounded), n_pts))
    value, unit = gr.exact_reference(case)
    gr._REFERENCES.setdefault((big.name, "exact"), (gr.expand(value, n_pts), gr.expand(unit, n_pts)))
    return big


# ---- the kernel against the exact statement -----------------------------------------------------------------------------------------
REPORT: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        print("\ngeopotential on model levels, worst ulps of U from exact (kernel / numpy's float64 / bound):")
        for key, row in sorted(REPORT.items()):
            print(f"  {key:<60} kernel {row['kernel']:11.4f}   numpy {row['numpy_float64']:11.4f}   bound {row['bound']:.8g}")
        if os.environ.get("ATX_GEOPOTENTIAL_ULPS_JSON"):
            with open(os.environ["ATX_GEOPOTENTIAL_ULPS_JSON"], "w") as f:
                json.dump(dict(unit="ulps of U[k] = |zs| + sum below |delta r t| + |alpha r t| in the stack's type", kernel=REPORT), f, indent=1)
                f.write("\n")


@pytest.mark.parametrize("shape", gr.SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}pts-{'zs' if s[3] else 'nozs'}")
@pytest.mark.parametrize("T", WIDTHS)
def test_the_kernel_is_within_its_budget_of_the_exact_statement(dev, T, shape):
    """Every storage shape through the one comparison the host test plants defects in; the shapes are byte-identical to each other."""
    n_lev, kind, n_pts, with_zs = shape
    case = expanded(gr.make_case(T, n_lev, kind, with_zs), n_pts)
    first = None
    for storage in STORAGE:
        got = run_kernel(dev, case, storage, n_pts)
        if first is None:
            report: dict = {}
            gr.check(lambda c: got, [case], NUMPY_WORST_GEOPOTENTIAL, report)
            REPORT.update(report)
            first = got
        else:
            assert got.tobytes() == first.tobytes(), f"{case.name}: {storage} differs from {STORAGE[0]}"


@pytest.mark.parametrize("T", WIDTHS)
def test_model_level_zero_alone_is_the_restatement_bit_for_bit(dev, T):
    """n_lev = 1 with n_half = 2: alpha = ln 2, no logarithm, no pressure — a NaN sp does not reach it."""
    for with_zs in (True, False):
        case = gr.make_case(T, 1, gr.WHOLE, with_zs)
        assert not gr.has_logarithm(case) and case.n_half == 2
        for storage in STORAGE:
            got = run_kernel(dev, case, storage, case.n_pts)
            gr.assert_same_bits(got, gr.reference(case), f"{case.name} {storage}")
            assert np.isfinite(got[4, 0]) and np.isnan(case.sp[4])


@pytest.mark.parametrize("T", WIDTHS)
def test_special_values_are_where_the_restatement_has_them(dev, T):
    """A NaN planted mid-column reaches its level and every level above, nothing below; a NaN sp the whole column."""
    case = gr.make_case(T, 60, gr.SUBSET)
    want = gr.reference(case)
    mid = case.n_lev // 2
    for storage in ("columns", "fields"):
        got = run_kernel(dev, case, storage, case.n_pts)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
        for column in (1, 5):
            assert np.isnan(got[column, : mid + 1]).all() and np.isfinite(got[column, mid + 1:]).all()
        assert np.isposinf(got[2, 0]) and np.isfinite(got[2, 1:]).all() and np.isnan(got[3]).all() and np.isnan(got[4]).all()


def test_without_zs_the_bottom_row_is_its_own_term(dev):
    """zs == NULL: the bottom row is (alpha r) t of that level; the same call with a zs of zeros gives the same bytes."""
    case = gr.make_case(np.float64, 3, gr.WHOLE, with_zs=False)
    got = run_kernel(dev, case, "columns", case.n_pts)
    zeros = gr.GeoCase(case.name + "-zeros", case.T, case.A, case.B, case.sp, np.zeros_like(case.sp), case.t, case.q)
    assert run_kernel(dev, zeros, "columns", case.n_pts).tobytes() == got.tobytes()


# ---- the layer below the filter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [COLUMNS, FIELDS], ids=["columns", "fields"])
def test_geopotential_on_model_levels_takes_two_stacks(dev, layout):
    case = gr.make_case(np.float32, 60, gr.SUBSET)
    t = Stack.from_fields(list(case.t.T), dev=dev, layout=layout)
    q = Stack.from_fields(list(case.q.T), dev=dev, layout=layout)
    out = geopotential_on_model_levels(t, q, torch.from_numpy(case.sp).to(dev), torch.from_numpy(case.zs).to(dev), case.A, case.B)
    assert (out.n_pts, out.n_lev, out.layout, out.dtype) == (case.n_pts, 60, layout, torch.float32)
    gr.check(lambda c: np.ascontiguousarray(out.numpy().T), [case], NUMPY_WORST_GEOPOTENTIAL)


# ---- the filter, end to end --------------------------------------------------------------------------------------------------------------
N_LEV = 17
LEVELS = [1000, 850, 500, 200, 50]  # hPa
DATES = (20260101, 20260102)


def small_world(dtype=np.float64):
    grid = lookup([10.0, 10.0])  # 684 points: more than one workgroup in either layout, and few enough for the exact evaluator
    lat, lon = np.asarray(grid["latitudes"], dtype=np.float64), np.asarray(grid["longitudes"], dtype=np.float64)
    n = len(lat)
    rng = np.random.default_rng(23)
    A, B = gr.eta_table(N_LEV + 1)
    specs, cases = [], {}
    for date in DATES:
        common = dict(latitudes=lat, longitudes=lon, date=date, time=0, step=0)
        sp = rng.uniform(50000.0, 105000.0, n).astype(dtype)
        zs = rng.uniform(-500.0, 30000.0, n).astype(dtype)
        t = (250.0 + 30.0 * rng.standard_normal((n, N_LEV))).astype(dtype)
        q = rng.uniform(0.0, 0.02, (n, N_LEV)).astype(dtype)
        specs.append(dict(values=(280.0 + rng.standard_normal(n)).astype(dtype), param="2t", levtype="sfc", **common))
        specs.append(dict(values=zs, param="z", levtype="ml", levelist=1, **common))  # as MARS keeps it
        for level in rng.permutation(N_LEV) + 1:  # the levels in no order
            specs.append(dict(values=t[:, level - 1].copy(), param="t", levtype="ml", levelist=int(level), **common))
            specs.append(dict(values=q[:, level - 1].copy(), param="q", levtype="ml", levelist=int(level), **common))
        specs.append(dict(values=sp, param="sp", levtype="sfc", **common))
        cases[date] = gr.GeoCase(f"world-{date}-{np.dtype(dtype).name}", dtype, A, B, sp, zs, t, q)
    return fieldlist_from_dicts(specs, mars=True), cases, dict(A=A.tolist(), B=B.tolist())


def assert_within(got: np.ndarray, case: gr.GeoCase, what: str) -> None:
    """Within the bound that numpy's own worst error ON THIS CASE gives (measured here, on the CPU, as the pinned ones were)."""
    value, unit = gr.exact_reference(case)
    e = gr.errors(got, value, unit)
    limit = gr.bound(case, gr.numpy_worst(case))
    assert np.nanmax(e) <= limit, f"{what}: {np.nanmax(e):.4f} ulps of U from exact > {limit:.6g}"


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_filter_end_to_end(dev, monkeypatch, dtype):
    data, cases, AB = small_world(dtype)
    f = create_filter_by_name("geopotential_on_model_levels", model_level_AB=AB)
    launches = []
    real = native_geopotential.geopotential
    monkeypatch.setattr(native_geopotential, "geopotential", lambda *a, **k: (launches.append(k["n_lev"]), real(*a, **k))[1])
    result = list(f.forward(data))
    assert launches == [N_LEV, N_LEV]  # ONE launch per group
    kept = [g for g in data if g.metadata("param") != "z"]  # the surface z is (z, ml, 1): the output's level 1 takes its place
    assert all(a is b for a, b in zip(result, kept)) and len(result) == len(kept) + len(DATES) * N_LEV
    new = result[len(kept):]
    assert [(g.metadata("date"), g.metadata("param"), g.metadata("levtype"), g.metadata("levelist")) for g in new] == [
        (date, "z", "ml", level) for date in DATES for level in range(1, N_LEV + 1)]
    assert len({id(g.stack_ref()[0]) for g in new}) == len(DATES) and all(g.stack_ref()[0].data.is_cuda for g in new)  # levels of one resident stack
    assert all(g.stack_ref()[0].dtype == (torch.float32 if dtype is np.float32 else torch.float64) for g in new)
    assert new[0].metadata(namespace="mars")["levelist"] == 1 and new[0].metadata(namespace="mars")["param"] == "z"
    for i, date in enumerate(DATES):
        got = np.stack([g.to_numpy(flatten=True) for g in new[i * N_LEV:(i + 1) * N_LEV]], axis=1)
        assert got.dtype == dtype
        assert_within(got, cases[date], f"filter, {date}")


def test_one_float64_field_makes_the_result_float64(dev):
    data, cases, AB = small_world(np.float32)
    fields = list(data)
    i = next(i for i, g in enumerate(fields) if g.metadata("param") == "sp" and g.metadata("date") == DATES[0])
    fields[i] = fields[i].clone(values=fields[i].to_numpy(flatten=True).astype(np.float64))
    new = [g for g in create_filter_by_name("geopotential_on_model_levels", model_level_AB=AB, output="zml").forward(FieldList(fields))
           if g.metadata("param") == "zml"]
    assert [g.stack_ref()[0].dtype for g in new[:N_LEV]] == [torch.float64] * N_LEV
    assert [g.stack_ref()[0].dtype for g in new[N_LEV:]] == [torch.float32] * N_LEV


def test_geopotential_then_ml_to_pl_never_leaves_hbm(dev):
    """``geopotential_on_model_levels | ml_to_pl(params=["z"])`` against the two restatements composed.  The interpolation is a convex
    combination of two levels of z (w inside [0, 1] up to its rounding) or a copy of one: the kernel's z is within ``bound`` of exact and
    numpy's within its pinned worst, both in ulps of U, U grows towards the top and z <= U — so the two results differ by at most
    bound + worst ulps of the upper level's U, and the three roundings of y = a + w (b - a), each at most an ulp of U."""
    data, cases, AB = small_world(np.float64)
    chain = create_filter_by_name("geopotential_on_model_levels", model_level_AB=AB) | create_filter_by_name("ml_to_pl", levels=LEVELS, model_level_AB=AB,
                                                                                                           params=["z"])
    got = [g for g in chain.forward(data) if g.metadata("levtype") == "pl"]
    assert [(g.metadata("date"), g.metadata("param"), g.metadata("levelist")) for g in got] == [(d, "z", v) for d in DATES for v in LEVELS]
    assert all(g.stack_ref() is not None and g.stack_ref()[0].data.is_cuda for g in got)
    for i, date in enumerate(DATES):
        case = cases[date]
        z = gr.reference(case)
        composed = lr.restate(lr.LevelsCase(f"z-{date}", np.float64, case.A, case.B, None, case.sp, z[:, None, :], np.array([100.0 * v for v in LEVELS])))
        _, unit = gr.exact_reference(case)
        top_unit = np.array([float(u) for u in unit[:, 0]])  # one ulp of U of the top level: the largest of the column
        worst = gr.numpy_worst(case)  # numpy's own, on this case
        limit = (gr.bound(case, worst) + worst + 3.0) * top_unit
        for j, level in enumerate(LEVELS):
            apart = np.abs(got[i * len(LEVELS) + j].to_numpy(flatten=True) - composed[:, 0, j])
            assert (apart <= limit).all(), (date, level, float((apart / top_unit).max()))


def test_fields_given_in_the_fields_layout_give_the_same_bits(dev):
    data, cases, AB = small_world(np.float64)
    f = create_filter_by_name("geopotential_on_model_levels", model_level_AB=AB)
    host = list(data)
    stack = Stack.from_fields([g.to_numpy(flatten=True) for g in host], dev=dev, layout=FIELDS)
    resident = FieldList([new_field_from_stack(stack, i, template=g) for i, g in enumerate(host)])
    a = [g for g in f.forward(data) if g.metadata("param") == "z"]
    b = [g for g in f.forward(resident) if g.metadata("param") == "z"]
    assert len(a) == len(b) == len(DATES) * N_LEV
    assert all(g.stack_ref()[0].layout == COLUMNS for g in a) and all(g.stack_ref()[0].layout == FIELDS for g in b)
    for x, y in zip(a, b):
        assert (x.metadata("date"), x.metadata("levelist")) == (y.metadata("date"), y.metadata("levelist"))
        assert x.to_numpy(flatten=True).tobytes() == y.to_numpy(flatten=True).tobytes(), "FIELDS against COLUMNS"
