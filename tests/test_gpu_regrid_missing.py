"""Missing-value-aware regridding on the device: ``atx_regrid_ell_missing`` / ``atx_regrid_csr_missing`` against the restatement
(tests/regrid_missing_restatement.py) — bit for bit on every element that is a number, NaN for NaN, none left out — through the checks
of tests/regrid_missing_checks.py, then ``GatherPlan.apply(missing=)`` and the ``regrid`` filter's ``missing=`` above them.

The forms of csrc/missing/atx_regrid_missing.hip and the k that reaches each (``launch_ell_missing``): compile-time rows k = 1, 2, 3, 4, 8, 16;
the run-time loop for every other k (here 5, 6, 17) and for CSR rows; each with 16-byte vectors ("tight", "loose") and single elements
("odd-pitch", "offset"), in float32 and float64.  ``LADDER`` is read from the source, so a new compile-time form without a case fails here.
"""

from __future__ import annotations

import os
import re

import numpy as np
import pytest
import torch

from anemoi_transform_amd import interp, native, native_missing
from anemoi_transform_amd.fields import FieldList, new_field_from_stack
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.gather import GatherPlan
from anemoi_transform_amd.grids import lookup
from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack

import regrid_missing_restatement as rs
from regrid_missing_checks import Kernels, canary, check_case
from test_filters import test_source

pytestmark = pytest.mark.gpu

F32_LEVELS = (1, 3, 4, 5, 8, 9, 25)  # every n_lev % VEC, n_lev < VEC
F64_LEVELS = (1, 2, 3, 25)
KS = (1, 2, 3, 4, 5, 8, 16, 17)
CONFIGS = ((rs.ALL, 0.0), (rs.HEAVIEST, 0.0), (rs.ALL, 0.5), (rs.HEAVIEST, 1.0), (rs.ALL, 1.0), (rs.HEAVIEST, 0.5))
WIDTHS = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]


def ladder() -> tuple:
    path = os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc", "missing", "atx_regrid_missing.hip")
    return tuple(int(k) for k in re.findall(r"case (\d+): return launch\(IntTag<\1>\{\}\);", open(path).read()))


@pytest.fixture(scope="module")
def kern(dev) -> Kernels:
    return Kernels(native_missing.regrid_ell_missing, native_missing.regrid_csr_missing, upload=lambda a: torch.from_numpy(a).to(dev),
                   download=lambda t: t.cpu().numpy(), address=lambda t: t.data_ptr())


def test_every_compile_time_form_has_its_k_among_the_cases():
    assert ladder() == (1, 2, 3, 4, 8, 16) and set(ladder()) <= set(KS) and set(KS) - set(ladder()) == {5, 17}


@pytest.mark.parametrize("T", WIDTHS)
@pytest.mark.parametrize("k", KS)
def test_fixed_k_rows_at_every_level_count(kern, T, k):
    """Vector form: every k of the ladder, 5 and 17 on the loop, every n_lev % VEC, both policies, min_valid 0, 0.5 and 1."""
    for i, n_lev in enumerate(F32_LEVELS if T is np.float32 else F64_LEVELS):
        case = rs.make_case(T, k, n_lev)
        for j in (0, 1):
            policy, min_valid = CONFIGS[(KS.index(k) + 2 * i + j) % len(CONFIGS)]
            check_case(kern, case, policy, min_valid, ("tight", "loose")[(i + j) % 2])


@pytest.mark.parametrize("T", WIDTHS)
def test_the_scalar_form_at_every_k(kern, T):
    """Single elements: a base one element off the 16-byte boundary, and a pitch of n_lev + 1 that is no whole number of vectors."""
    n_lev = 5 if T is np.float32 else 2
    for i, k in enumerate(KS):
        case = rs.make_case(T, k, n_lev)
        check_case(kern, case, *CONFIGS[i % len(CONFIGS)], "offset")
        check_case(kern, case, *CONFIGS[(i + 3) % len(CONFIGS)], "odd-pitch")
    case = rs.make_case(T, 4, 25 if T is np.float32 else 3)
    check_case(kern, case, rs.HEAVIEST, 0.5, "offset")


@pytest.mark.parametrize("T", WIDTHS)
def test_target_counts_around_a_wave_and_a_workgroup(kern, T):
    for i, n_tgt in enumerate((1, 63, 64, 65, 131)):
        for k, n_lev in ((4, 5), (17, 3), (1, 4)):
            case = rs.make_case(T, k, n_lev, n_tgt=n_tgt)
            check_case(kern, case, *CONFIGS[(i + k) % len(CONFIGS)], ("tight", "offset", "loose")[i % 3])
    # 256 lanes per workgroup: items on the boundary and one past it (one vector per target)
    for n_tgt in (256, 257):
        check_case(kern, rs.make_case(T, 2, 16 // np.dtype(T).itemsize, n_tgt=n_tgt), rs.HEAVIEST, 0.5, "tight")


@pytest.mark.parametrize("T", WIDTHS)
def test_padded_rows(kern, T):
    """Absent entries anywhere in the row: the all-absent row (0), the full row, a single entry in the last slot; their weights unused."""
    for i, (k, n_lev) in enumerate(((3, 5), (4, 3), (6, 9), (8, 4), (16, 3))):
        case = rs.make_case(T, k, n_lev, padded=True)
        assert (case.idx[0] < 0).all() and (case.idx[1] >= 0).all() and (case.idx[2] >= 0).tolist() == [False] * (k - 1) + [True]
        for j, form in enumerate(("tight", "offset")):
            check_case(kern, case, *CONFIGS[(2 * i + j) % len(CONFIGS)], form)
        check_case(kern, case, rs.ALL, 0.5, "loose")  # (an absent entry's weight counted in tot shows here)


@pytest.mark.parametrize("T", WIDTHS)
def test_csr_rows(kern, T):
    lengths = [0, 70, 1, 4, 5, 0] + [3, 0, 5, 2, 9] * 25
    for i, n_lev in enumerate((F32_LEVELS if T is np.float32 else F64_LEVELS)):
        case = rs.make_case(T, 0, n_lev, lengths=lengths)
        check_case(kern, case, *CONFIGS[i % len(CONFIGS)], ("tight", "loose")[i % 2], "csr")
        check_case(kern, case, *CONFIGS[(i + 1) % len(CONFIGS)], "offset", "csr")
    check_case(kern, rs.make_case(T, 0, 5 if T is np.float32 else 2, lengths=lengths), rs.HEAVIEST, 0.5, "odd-pitch", "csr")
    for n_tgt, some in ((1, [3]), (1, [0]), (64, [2, 6] * 32), (65, [1] * 65)):
        check_case(kern, rs.make_case(T, 0, 5, n_tgt=n_tgt, lengths=some), rs.ALL, 0.5, "tight", "csr")


def test_validation_mode_refuses_a_table_that_points_outside_the_stack(dev):
    """ATX_VALIDATE=1, in a fresh process (tests/regrid_missing_validate_child.py: the variable is read once): the tables are
    range-checked on the device by the check libatx uses (csrc/atx_regrid_check.hpp) and a launch is refused, with the exact count of
    bad entries and nothing written, instead of reading outside the stack.  Tables of 7 x 3 = 21 entries (under one wave) and of
    300 x 4 = 1200 (no multiple of 64 or 256: several waves and a partial last one); per table a bad entry at the first position, at the
    last and at three positions (three different waves in the long table), -2 under padded rows (-1 is accepted there and refused
    without), a bad CSR index and an indptr entry above nnz: 7 refusals each.  Valid tables run and equal atx_regrid_ell's bits."""
    import subprocess
    import sys

    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "regrid_missing_validate_child.py")
    run = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=120, env=dict(os.environ, ATX_VALIDATE="1"))
    assert run.returncode == 0 and "refused 14" in run.stdout, run.stdout + run.stderr[-3000:]


# ---- GatherPlan ---------------------------------------------------------------------------------------------------------------------
def plan_case(name, plan: GatherPlan, T, values: np.ndarray) -> rs.MissingCase:
    """The restatement's view of a plan: its natural-order table with the weights rounded to T; ``values`` is [n_lev, n_src]."""
    if plan.kind == "ell":
        idx, w = plan.index, plan.weights.astype(T)
    else:
        lengths = np.diff(plan.indptr)
        k = int(lengths.max())
        present = np.arange(k)[None, :] < lengths[:, None]
        idx, w = np.full((plan.n_tgt, k), -1, dtype=np.int32), np.zeros((plan.n_tgt, k), dtype=T)
        idx[present], w[present] = plan.indices, plan.data.astype(T)
    return rs.MissingCase(name, T, idx.shape[1], values.shape[0], plan.n_src, plan.n_tgt, idx, w, np.ascontiguousarray(values.T.astype(T)))


def assert_same(got: np.ndarray, want: np.ndarray, what) -> None:
    B = rs.bits_type(want.dtype.type)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(B)[~nan], want.view(B)[~nan]), what


@pytest.mark.parametrize("T", WIDTHS)
def test_a_complete_stack_takes_the_plain_routes_bits(dev, T):
    """Nothing missing: the new route equals ``GatherPlan.apply`` without a policy bit for bit — fixed k, padded rows and CSR."""
    rng = np.random.default_rng(5)
    n_src, n_tgt, n_lev = 400, 333, 9
    x = Stack.from_fields((280.0 + 50.0 * rng.standard_normal((n_lev, n_src))).astype(T), dev=dev)
    lengths = rng.integers(0, 40, n_tgt)
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    plans = [GatherPlan(n_src, n_tgt, index=rng.integers(0, n_src, (n_tgt, k)), weights=rng.standard_normal((n_tgt, k))) for k in (1, 2, 4, 7, 11, 16, 17)]
    plans.append(GatherPlan(n_src, n_tgt, csr=(rng.standard_normal(indptr[-1]), rng.integers(0, n_src, indptr[-1]).astype(np.int32), indptr)))
    assert plans[4].padded and plans[4].k == 12 and plans[-1].kind == "csr"
    for plan in plans:
        want = plan.apply(x).numpy()
        for policy, min_valid in ((rs.ALL, 0.0), (rs.HEAVIEST, 1.0)):
            got = plan.apply(x, missing=policy, min_valid=min_valid).numpy()
            assert np.array_equal(got.view(rs.bits_type(T)), want.view(rs.bits_type(T))), (plan.kind, plan.k, policy)


def test_a_source_row_beyond_two_to_the_31_elements(dev):
    """float32, pitch 1024: the last source rows start past element 2^31 — offsets are 64-bit.  Only the rows the table names are touched."""
    n_src, pitch, n_lev, T = 2**21 + 8, 1024, 5, np.float32
    named = np.array([0, 7, 2**21 - 1, 2**21, 2**21 + 1, n_src - 2, n_src - 1])
    assert (n_src - 1) * pitch > 2**31
    small = rs.make_case(T, 4, n_lev, n_src=named.size, n_tgt=9, seed=31, name="beyond-2-31")
    src = torch.empty((n_src, pitch), dtype=torch.float32, device=dev)
    src[torch.from_numpy(named).to(dev), :n_lev] = torch.from_numpy(small.src).to(dev)
    idx = torch.from_numpy(named[small.idx].astype(np.int32).reshape(-1)).to(dev)
    w = torch.from_numpy(small.w.reshape(-1)).to(dev)
    out = torch.from_numpy(canary(T, small.n_tgt * 8).copy()).to(dev)
    for policy, min_valid in ((rs.ALL, 0.0), (rs.HEAVIEST, 0.5)):
        native_missing.regrid_ell_missing(src, out, idx, w, n_src=n_src, n_tgt=small.n_tgt, k=4, n_lev=n_lev, src_pitch=pitch, out_pitch=8, layout=COLUMNS,
                                  policy=policy, min_valid=min_valid)
        want, _ = rs.restated(small, policy, min_valid)
        assert_same(out.cpu().numpy().reshape(small.n_tgt, 8)[:, :n_lev].copy(), want, policy)
    del src


def test_apply_argument_errors_and_the_other_entry_points(dev):
    rng = np.random.default_rng(8)
    plan = GatherPlan(50, 20, index=rng.integers(0, 50, (20, 3)), weights=rng.random((20, 3)))
    values = rng.standard_normal((4, 50))
    values[rng.random(values.shape) < 0.4] = np.nan
    x = Stack.from_fields(values, dev=dev)
    want, _ = rs.restate(plan_case("entry-points", plan, np.float64, values), rs.ALL, 0.25)
    prog = native.level_program([[(native.OP_MUL, 0, 2.0, 0.0)] * 4], dev)
    with pytest.raises(ValueError, match="program"):
        plan.apply(x, prog=prog, n_stage=1, missing="all")
    with pytest.raises(ValueError, match="missing="):
        plan.apply(x, missing="some")
    with pytest.raises(ValueError, match="min_valid"):
        plan.apply(x, missing="all", min_valid=2.0)
    kept = x.new_like(n_pts=20)
    assert plan.apply(x, missing="all", min_valid=0.25, out=kept) is kept
    assert_same(kept.numpy().T.copy(), want, "out=")
    launch, out = plan.bind(x, missing="all", min_valid=0.25)
    launch()
    assert_same(out.numpy().T.copy(), want, "bind")
    for got in plan.apply_many([x, x], missing="all", min_valid=0.25):
        assert_same(got.numpy().T.copy(), want, "apply_many")
    ordered = GatherPlan(50, 20, index=plan.index, weights=plan.weights).order_targets(rng.permutation(20))
    assert_same(ordered.apply(x, missing="all", min_valid=0.25).numpy().T.copy(), want, "the visiting order changes nothing")
    # a field-major stack goes through a column stack and back
    xf = Stack.from_fields(values, dev=dev, layout=FIELDS)
    got = plan.apply(xf, missing="all", min_valid=0.25)
    assert got.layout == FIELDS
    assert_same(got.numpy().T.copy(), want, "fields")
    # an unweighted k = 1 plan is a copy under every policy
    copy = GatherPlan(50, 20, index=rng.integers(0, 50, 20))
    assert np.array_equal(copy.apply(x, missing="heaviest", min_valid=1.0).numpy(), copy.apply(x).numpy(), equal_nan=True)


# ---- the filter ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_pair():
    src, tgt = lookup("o16"), lookup([20.0, 20.0])
    idx, w = interp.knn_inverse_distance(src, tgt, k=4)
    matrix = {**interp.ell_to_csr(idx, w, len(src["latitudes"])), "in_latitudes": src["latitudes"], "in_longitudes": src["longitudes"],
              "out_latitudes": tgt["latitudes"], "out_longitudes": tgt["longitudes"]}
    return src, tgt, matrix


def specs_on(grid, T, n_fields=5, seed=3):
    rng = np.random.default_rng(seed)
    m = len(grid["latitudes"])
    specs = []
    for i in range(n_fields):
        values = (250.0 + 60.0 * rng.random(m)).astype(T)
        values[rng.random(m) < (0.0, 0.3, 0.7, 1.0, 0.1)[i % 5]] = np.nan
        specs.append({"param": "t", "levelist": i + 1, "values": values, "latitudes": grid["latitudes"], "longitudes": grid["longitudes"], "units": "K",
                      "valid_datetime": "2020-01-01T00:00:00Z"})
    return specs


def values_of(fields) -> np.ndarray:
    return np.stack([f.to_numpy(flatten=True) for f in fields])


@pytest.mark.parametrize("T", WIDTHS)
@pytest.mark.parametrize("spelling,policy", [("missing-if-all-missing", rs.ALL), ("missing-if-heaviest-missing", rs.HEAVIEST)])
def test_regrid_filter_with_a_matrix(dev, grid_pair, T, spelling, policy, monkeypatch):
    src, tgt, matrix = grid_pair
    specs = specs_on(src, T)
    host = test_source(specs).ds
    f = create_filter_by_name("regrid", matrix=matrix, missing=spelling, min_valid=0.5)
    plan = f.interpolator.plan
    case = plan_case(f"filter-{T.__name__}", plan, T, np.stack([s["values"] for s in specs]))
    want, _ = rs.restate(case, policy, 0.5)
    assert_same(values_of(f.forward(host)).T.copy(), want, "host fields")
    # a device-resident stack (the fields of a first regrid onto their own grid)
    resident = create_filter_by_name("regrid", in_grid=src, out_grid=src, method="nearest").forward(host)
    assert_same(values_of(f.forward(resident)).T.copy(), want, "resident stack")
    # a field-major stack
    stack = Stack.from_fields([s["values"] for s in specs], dev=dev, layout=FIELDS)
    on_fields = FieldList([new_field_from_stack(stack, level, template=t) for level, t in enumerate(host)])
    assert_same(values_of(f.forward(on_fields)).T.copy(), want, "field-major stack")
    # one shard of three
    sharded = create_filter_by_name("regrid", matrix=matrix, missing=spelling, min_valid=0.5, shard=(1, 3))
    lo, hi = plan.shard_range(1, 3)
    assert 0 < lo < hi < plan.n_tgt
    assert_same(values_of(sharded.forward(resident)).T.copy(), want[lo:hi], "shard (1, 3)")
    # followed by rescale in a pipeline: the regrid runs alone, fused or not the values are numpy's x * scale + offset of the regridded ones
    scaled = (want * T(2.0) + T(-273.15)).astype(T)
    for no_fusion in (False, True):
        if no_fusion:
            monkeypatch.setenv("ATX_NO_FUSION", "1")
        else:
            monkeypatch.delenv("ATX_NO_FUSION", raising=False)
        pipeline = create_filter_by_name("regrid", matrix=matrix, missing=spelling, min_valid=0.5) | create_filter_by_name("rescale", scale=2.0, offset=-273.15, param="t")
        assert_same(values_of(pipeline.forward(resident)).T.copy(), scaled, f"pipeline, ATX_NO_FUSION={no_fusion}")
    # missing-if-any-missing is the plain route
    plain = values_of(create_filter_by_name("regrid", matrix=matrix).forward(resident))
    assert_same(values_of(create_filter_by_name("regrid", matrix=matrix, missing="missing-if-any-missing").forward(resident)), plain, "any-missing")


def test_nearest_is_the_same_under_every_policy(grid_pair):
    src, tgt, _ = grid_pair
    host = test_source(specs_on(src, np.float64)).ds
    plain = values_of(create_filter_by_name("regrid", in_grid=src, out_grid=tgt, method="nearest").forward(host))
    assert np.isnan(plain).any() and not np.isnan(plain).all()
    for spelling in ("missing-if-all-missing", "missing-if-heaviest-missing"):
        got = values_of(create_filter_by_name("regrid", in_grid=src, out_grid=tgt, method="nearest", missing=spelling, min_valid=1.0).forward(host))
        assert_same(got, plain, spelling)


def test_a_coastline_keeps_its_sea_points():
    """0.25 degree -> 1 degree, method="linear", a NaN half-plane east of 180.1 E: with missing-if-all-missing exactly the targets whose
    sources are all NaN come out NaN (counted on the host from the plan's table); without a policy every target that touches a NaN does."""
    src = lookup([0.25, 0.25])
    lon = np.asarray(src["longitudes"])
    values = 280.0 + 10.0 * np.cos(np.radians(np.asarray(src["latitudes"]))) + 0.01 * lon
    land = lon > 180.1
    values[land] = np.nan
    specs = [{"param": "sst", "levelist": 1, "values": values, "latitudes": src["latitudes"], "longitudes": src["longitudes"], "units": "K",
              "valid_datetime": "2020-01-01T00:00:00Z"}]
    host = test_source(specs).ds
    f = create_filter_by_name("regrid", in_grid=[0.25, 0.25], out_grid=[1.0, 1.0], method="linear", missing="missing-if-all-missing")
    plan = f.interpolator.plan
    assert plan.kind == "ell"
    present = plan.index >= 0
    is_land = np.where(present, land[np.where(present, plan.index, 0)], False)
    all_land = (is_land | ~present).all(axis=1) & present.any(axis=1)
    any_land = is_land.any(axis=1)
    assert 0 < all_land.sum() < any_land.sum() < plan.n_tgt
    got = f.forward(host)[0].to_numpy(flatten=True)
    assert np.array_equal(np.isnan(got), all_land) and int(np.isnan(got).sum()) == int(all_land.sum())
    want, _ = rs.restate(plan_case("coastline", plan, np.float64, values[None, :]), rs.ALL, 0.0)
    assert_same(got[:, None].copy(), want, "coastline")
    plain = create_filter_by_name("regrid", in_grid=[0.25, 0.25], out_grid=[1.0, 1.0], method="linear").forward(host)[0].to_numpy(flatten=True)
    assert np.array_equal(np.isnan(plain), any_land)
    sea = ~any_land
    assert np.array_equal(got[sea], plain[sea])  # where nothing is missing: the plain route's bits
