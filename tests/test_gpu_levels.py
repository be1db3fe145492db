"""Model levels to pressure levels on the device: ``atx_levels_interpolate`` against the restatement of include/atx_levels.h
(tests/levels_restatement.py) — bit for bit for the linear coordinate, in every storage shape and under both ``outside`` policies; within
the budget of ``levels_restatement.log_budget`` of the exact statement for the log coordinate, which goes through the library's own
logarithm — and the ``ml_to_pl`` filter end to end.

Worst distance from exact measured on an MI355X, log coordinate, in ulps of max(|x[a]|, |x[b]|) (profiles/levels_ulps.json, "kernel"):
float64 39.76 on the base case (numpy's own arithmetic: 39.76, bound 81.53), 22.29 on the cut table (bound 46.59), 13.06 on the subset
column (bound 28.12); float32 at most 0.49996 (bound 0.5000001: one rounding and 2^-29 of the float64 bound) — the same in every storage
route.  The test prints the figures of its run, and writes them as JSON to the file that ``ATX_LEVELS_ULPS_JSON`` names, if it is set.
"""

from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import levels_restatement as lr
from anemoi_transform_amd import native_levels
from anemoi_transform_amd.fields import fieldlist_from_dicts, new_field_from_stack
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.grids import lookup
from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack
from anemoi_transform_amd.vertical import interpolate_levels
from hybrid_column_common import CANARY, COLUMN_STORAGE, FIELD_STORAGE, WIDTHS, allocate

pytestmark = pytest.mark.gpu

STORAGE = COLUMN_STORAGE + FIELD_STORAGE


def run_kernel(dev, case: lr.LevelsCase, storage: str, coordinate: str, outside: str) -> np.ndarray:
    """The kernel on the case in one storage shape: ``[n_pts, n_var, n_tgt]``.  Asserts that nothing is written outside the
    ``n_var x n_tgt`` rows of a point and that the source stack is left as it was."""
    n_pts, n_var, n_lev, n_tgt = case.n_pts, case.n_var, case.n_lev, case.n_tgt
    columns = storage.startswith("columns")
    layout = COLUMNS if columns else FIELDS
    rows_in, rows_out = n_var * n_lev, n_var * n_tgt
    values = np.ascontiguousarray(case.x.reshape(n_pts, rows_in))
    src = allocate(n_pts, rows_in, storage, case.T, dev, float("nan")) if columns else allocate(rows_in, n_pts, storage, case.T, dev, float("nan"))
    out = allocate(n_pts, rows_out, storage, case.T, dev, CANARY) if columns else allocate(rows_out, n_pts, storage, case.T, dev, CANARY)
    if n_pts:
        if columns:
            src[:, :rows_in] = torch.from_numpy(values).to(dev)
        else:
            src[:, :n_pts] = torch.from_numpy(np.ascontiguousarray(values.T)).to(dev)
    before = src.clone()
    f64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    native_levels.interpolate(src, out, torch.from_numpy(case.sp).to(dev), f64(case.A), f64(case.B), f64(case.targets), n_pts=n_pts, n_var=n_var,
                              n_lev=n_lev, n_tgt=n_tgt, src_pitch=src.stride(0), out_pitch=out.stride(0), layout=layout,
                              level_index=None if case.m is None else case.m.tolist(), coordinate=coordinate, outside=outside)
    torch.cuda.synchronize()
    bits = torch.int32 if case.T is np.float32 else torch.int64
    assert torch.equal(src.view(bits), before.view(bits)), f"{case.name} {storage}: the source stack was modified"
    host = out.cpu().numpy()
    if columns:
        assert (host[:, rows_out:] == CANARY).all(), f"{case.name} {storage}: written beyond a point's {rows_out} rows"
        return host[:, :rows_out].reshape(n_pts, n_var, n_tgt).copy()
    assert (host[:, n_pts:] == CANARY).all(), f"{case.name} {storage}: written beyond the {n_pts} points of a row"
    return np.ascontiguousarray(host[:, :n_pts].T).reshape(n_pts, n_var, n_tgt)


def all_cases(T) -> list:
    return lr.edge_cases(T) + [lr.shape_case(T, *shape) for shape in lr.SHAPES]


# ---- bit equality with the restatement ------------------------------------------------------------------------------------------------
def test_the_base_case_reaches_every_class_of_the_statement():
    """Asserted before anything is compared: at least a quarter of the base case's outputs are interior, and none of the four classes is
    empty (checked on a CPU: 48 % interior, 10 % above the top, 3.4 % in the lowest half layer, 38.5 % below the ground)."""
    shares = lr.base_class_shares(np.float64)
    print("base case:", {k: round(v, 4) for k, v in shares.items()})
    assert shares[lr.INTERIOR] >= 0.25 and all(shares[c] > 0 for c in lr.CLASSES), shares
    assert lr.on_a_full_level(lr.base_case(np.float64)).sum() >= 5  # the targets added on top: equal to a point's p_full


@pytest.mark.parametrize("index", range(4 + len(lr.SHAPES)), ids=lambda i: (["base", "subset", "cut", "bent"] + ["x".join(map(str, s)) for s in lr.SHAPES])[i])
@pytest.mark.parametrize("T", WIDTHS)
def test_linear_is_the_restatement_bit_for_bit(dev, T, index):
    """Every storage shape and both policies against the one restatement: the 16-byte route, the scalar route and the field-major
    kernel therefore also equal each other."""
    case = all_cases(T)[index]
    for outside in (lr.NEAREST, lr.MISSING):
        want = lr.reference(case, lr.LINEAR, outside)
        for storage in STORAGE:
            lr.assert_same_bits(run_kernel(dev, case, storage, lr.LINEAR, outside), want, f"{case.name} {storage} {outside}")


def test_the_comparison_is_the_one_the_host_test_plants_defects_in(dev):
    lr.check_linear(lambda case, c, o: run_kernel(dev, case, "columns", c, o), lr.edge_cases(np.float64)[1:])


# ---- the log coordinate ----------------------------------------------------------------------------------------------------------------
LOG_REPORT: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if LOG_REPORT:
        print("\nlevel interpolation, log coordinate, worst ulps of max(|x[a]|, |x[b]|) from exact (kernel / numpy's float64 / bound):")
        for key, row in sorted(LOG_REPORT.items()):
            print(f"  {key:<60} kernel {row['kernel']:9.4f}   numpy {row['numpy_float64']:9.4f}   bound {row['bound']:.6g}")
        if os.environ.get("ATX_LEVELS_ULPS_JSON"):
            with open(os.environ["ATX_LEVELS_ULPS_JSON"], "w") as f:
                json.dump(LOG_REPORT, f, indent=1)


@pytest.mark.parametrize("storage", ["columns", "columns-pitch+1", "fields"])
@pytest.mark.parametrize("T", WIDTHS)
def test_log_is_within_its_budget_of_the_exact_statement(dev, T, storage):
    report: dict = {}
    lr.check_log(lambda case, c, o: run_kernel(dev, case, storage, c, o), lr.log_cases(T), report)
    for name, row in report.items():
        LOG_REPORT[f"{name} {storage}"] = row


@pytest.mark.parametrize("T", WIDTHS)
def test_log_routes_agree_bit_for_bit(dev, T):
    for case in (lr.base_case(T), lr.edge_cases(T)[3]):  # the bent columns too: the FIELDS kernel counts every column level by level
        first = run_kernel(dev, case, STORAGE[0], lr.LOG, lr.MISSING)
        for storage in STORAGE[1:]:
            lr.assert_same_bits(run_kernel(dev, case, storage, lr.LOG, lr.MISSING), first, f"{case.name} log {storage}")


# ---- the layer below the filter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [COLUMNS, FIELDS], ids=["columns", "fields"])
def test_interpolate_levels_takes_a_tall_stack(dev, layout):
    case = lr.shape_case(np.float32, 65, 17, 13, 3, "subset")
    stack = Stack.from_fields(list(case.x.reshape(case.n_pts, -1).T), dev=dev, layout=layout)
    out = interpolate_levels(stack, torch.from_numpy(case.sp).to(dev), case.A, case.B, case.targets, n_var=3, level_index=case.m.tolist(),
                             outside="missing")
    assert (out.n_pts, out.n_lev, out.layout, out.dtype) == (65, 39, layout, torch.float32)
    lr.assert_same_bits(np.ascontiguousarray(out.numpy().T).reshape(65, 3, 13), lr.reference(case, lr.LINEAR, lr.MISSING), f"tall stack, layout {layout}")


# ---- the filter, end to end --------------------------------------------------------------------------------------------------------------
N_LEV = 17
LEVELS = [1000, 850, 500, 200, 50, 1]  # hPa: below the ground for some points, interior, above the top full level
DATES = (20260101, 20260102)


def small_world():
    grid = lookup("o32")
    lat, lon = np.asarray(grid["latitudes"], dtype=np.float64), np.asarray(grid["longitudes"], dtype=np.float64)
    n = len(lat)
    rng = np.random.default_rng(17)
    A, B = lr.eta_table(N_LEV + 1)
    specs, cases = [], {}
    for date in DATES:
        common = dict(latitudes=lat, longitudes=lon, date=date, time=0, step=0)
        sp = rng.uniform(50000.0, 105000.0, n)
        specs.append(dict(values=280.0 + rng.standard_normal(n), param="2t", levtype="sfc", **common))
        for level in rng.permutation(N_LEV) + 1:  # the levels in no order
            for param in ("t", "q"):
                cases.setdefault((date, param), np.empty((n, 1, N_LEV)))[:, 0, level - 1] = 250.0 + 30.0 * rng.standard_normal(n)
                specs.append(dict(values=cases[(date, param)][:, 0, level - 1].copy(), param=param, levtype="ml", levelist=int(level), **common))
        specs.append(dict(values=sp, param="sp", levtype="sfc", **common))
        for param in ("t", "q"):
            cases[(date, param)] = lr.LevelsCase(f"world-{date}-{param}", np.float64, A, B, None, sp, cases[(date, param)],
                                                 np.array([100.0 * v for v in LEVELS]))
    return fieldlist_from_dicts(specs, mars=True), cases, dict(A=A.tolist(), B=B.tolist())


@pytest.mark.parametrize("interpolation,outside", [("linear", "nearest"), ("linear", "missing")])
def test_the_filter_end_to_end(dev, monkeypatch, interpolation, outside):
    data, cases, AB = small_world()
    f = create_filter_by_name("ml_to_pl", levels=LEVELS, model_level_AB=AB, interpolation=interpolation, outside=outside)
    launches = []
    real = native_levels.interpolate
    monkeypatch.setattr(native_levels, "interpolate", lambda *a, **k: (launches.append(k["n_var"]), real(*a, **k))[1])
    result = list(f.forward(data))
    assert launches == [2, 2]  # t and q of a date share a level set: ONE launch per group, a tall stack of two variables
    kept = [g for g in data if g.metadata("levtype") != "ml"]
    assert len(result) == len(kept) + len(DATES) * 2 * len(LEVELS)
    assert all(a is b for a, b in zip(result, kept))  # every field that was not interpolated first, in input order, untouched, sp included
    new = result[len(kept):]
    expected = [(date, param, level) for date in DATES for param in ("t", "q") for level in LEVELS]
    assert [(g.metadata("date"), g.metadata("param"), g.metadata("levelist")) for g in new] == expected
    for g, (date, param, level) in zip(new, expected):
        assert g.metadata("levtype") == "pl" and g.metadata(namespace="mars")["levtype"] == "pl" and g.metadata(namespace="mars")["levelist"] == level
        assert g.stack_ref() is not None and g.stack_ref()[0].data.is_cuda  # resident
        assert g.shape == data[0].shape and np.array_equal(g.grid_points()[0], data[0].grid_points()[0])
        want = lr.reference(cases[(date, param)], interpolation, outside)[:, 0, LEVELS.index(level)]
        lr.assert_same_bits(g.to_numpy(flatten=True), want, f"{date} {param} {level} hPa")
    first_ml = {(g.metadata("date"), g.metadata("param")): g for g in reversed(list(data)) if g.metadata("levtype") == "ml"}
    assert all(g._template is first_ml[(date, param)] for g, (date, param, _) in zip(new, expected))  # the param's first ml field
    assert len({id(g.stack_ref()[0]) for g in new}) == len(DATES)  # one output stack per launch
    if outside == "missing":
        assert np.isnan(new[0].to_numpy()).any() and np.isnan(new[len(LEVELS) - 1].to_numpy()).all()  # below the ground; above the top


def test_ml_to_pl_then_regrid_never_leaves_hbm(dev):
    data, cases, AB = small_world()
    vertical = create_filter_by_name("ml_to_pl", levels=LEVELS, model_level_AB=AB, params=["t"])
    regrid = create_filter_by_name("regrid", in_grid="O32", out_grid=[5.0, 5.0], method="nearest")
    only = [g for g in data if g.metadata("param") in ("t", "sp")]
    got = [g for g in (vertical | regrid).forward(fieldlist_from_list(only)) if g.metadata("levtype") == "pl"]
    assert len(got) == len(DATES) * len(LEVELS) and all(g.stack_ref() is not None for g in got)
    # the same regrid applied to the restatement's output, field by field
    template = only[0]
    restated = [template.clone(values=lr.reference(cases[(date, "t")], lr.LINEAR, lr.NEAREST)[:, 0, t], param="t", levtype="pl", levelist=level, date=date)
                for date in DATES for t, level in enumerate(LEVELS)]
    want = list(regrid.forward(fieldlist_from_list(restated)))
    for g, w in zip(got, want):
        assert (g.metadata("date"), g.metadata("levelist")) == (w.metadata("date"), w.metadata("levelist"))
        lr.assert_same_bits(g.to_numpy(flatten=True), w.to_numpy(flatten=True), f"regrid of {g.metadata('date')} {g.metadata('levelist')} hPa")


def fieldlist_from_list(fields):
    from anemoi_transform_amd.fields import FieldList

    return FieldList(list(fields))


def test_fields_given_in_the_fields_layout_give_the_same_bits(dev):
    data, cases, AB = small_world()
    f = create_filter_by_name("ml_to_pl", levels=LEVELS, model_level_AB=AB, outside="missing")
    host = list(data)
    stack = Stack.from_fields([g.to_numpy(flatten=True) for g in host], dev=dev, layout=FIELDS)
    resident = fieldlist_from_list(new_field_from_stack(stack, i, template=g) for i, g in enumerate(host))
    a = [g for g in f.forward(data) if g.metadata("levtype") == "pl"]
    b = [g for g in f.forward(resident) if g.metadata("levtype") == "pl"]
    assert len(a) == len(b) == len(DATES) * 2 * len(LEVELS)
    assert all(g.stack_ref()[0].layout == COLUMNS for g in a) and all(g.stack_ref()[0].layout == FIELDS for g in b)
    for x, y in zip(a, b):
        assert (x.metadata("date"), x.metadata("param"), x.metadata("levelist")) == (y.metadata("date"), y.metadata("param"), y.metadata("levelist"))
        lr.assert_same_bits(y.to_numpy(flatten=True), x.to_numpy(flatten=True), "FIELDS against COLUMNS")
