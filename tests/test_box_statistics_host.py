"""Grid-box statistics without a GPU: the restatement of include/atx_stat.h (tests/box_statistics_restatement.py) against independent
routes — numpy's ``fmax`` / ``fmin`` ``.reduceat``, a dict of classes, exact rational arithmetic, the missing-value restatement's NaN
pattern — once as it is and once per planted defect; then the C ABI's argument validation through ctypes, and the Python layers'
errors (``GatherPlan.reduce``, the ``regrid`` filter's ``statistic=``)."""

from __future__ import annotations

import ctypes
import logging
import os
from fractions import Fraction

import numpy as np
import pytest

from anemoi_transform_amd import native, native_stat
from anemoi_transform_amd.filters import create_filter_by_name, fusion
from anemoi_transform_amd.gather import GatherPlan

import box_statistics_restatement as bs
import regrid_missing_restatement as ms

WIDTHS = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]


def rows_of(case: bs.StatCase):
    for t in range(case.n_tgt):
        lo, hi = int(case.indptr[t]), int(case.indptr[t + 1])
        yield t, case.indices[lo:hi], (None if case.data is None else case.data[lo:hi])


# ---- the independent routes: each returns nothing and asserts --------------------------------------------------------------------
def check_extremes_against_reduceat(T, defect=None):
    """Where the policy lets NaN drop (ALL, min_valid = 0), the maximum / minimum of a row are numpy's fmax / fmin over its gathered
    sources (values compared with ==: -0.0 and 0.0 are one extreme); an empty row is NaN."""
    for weighted in (True, False):
        case = bs.make_case(T, 6, weighted=weighted)
        gathered = case.src[case.indices]  # [nnz, n_lev]
        gathered = np.where(np.isnan(gathered), T(np.nan), gathered)  # (C's fmax may answer a signalling NaN with a NaN: quiet them all)
        lengths = np.diff(case.indptr)
        filled = np.flatnonzero(lengths > 0)
        for statistic, ufunc in ((bs.MAXIMUM, np.fmax), (bs.MINIMUM, np.fmin)):
            got = bs.restate(case, statistic, bs.ALL, 0.0, defect)
            with np.errstate(all="ignore"):
                want = ufunc.reduceat(gathered, case.indptr[:-1][filled], axis=0)
            assert np.isnan(got[lengths == 0]).all()
            assert np.array_equal(got[filled], want, equal_nan=True), (statistic, weighted)


def mode_by_classes(T, xs, ws):
    """A dict of classes: value -> weight, added in row order in T; the heaviest class, the smaller value among equals."""
    classes: dict = {}
    for x, w in zip(xs, ws):
        if x == x:
            classes[float(x)] = T(classes.get(float(x), T(0)) + w)
    if not classes:
        return T(np.nan)
    top = max(classes.values())
    return T(min(v for v, w in classes.items() if w == top))


def tie_cases(T):
    return [bs.rows_case(T, f"ties-{np.dtype(T).name}", [[1, 3], [3, 1], [2, 5, 2, 5], [5, 2, 5, 2], [7, 7, 7], [4, 9, 9]],
                         [[0.25, 0.25], [0.25, 0.25], [0.125, 0.25, 0.125, 0.25], [0.125, 0.25, 0.125, 0.25], [0.5, 0.25, 0.25], [0.5, 0.25, 0.125]])]


def check_mode_against_classes(T, defect=None):
    for case in [bs.make_case(T, 6, categorical=True)] + tie_cases(T):
        got = bs.restate(case, bs.MODE, bs.ALL, 0.0, defect)
        for t, idx, w in rows_of(case):
            for l in range(case.n_lev):
                want = mode_by_classes(T, case.src[idx, l], w)
                assert (np.isnan(want) and np.isnan(got[t, l])) or got[t, l] == want, (case.name, t, l, got[t, l], want)


def gamma(k: int, u: Fraction) -> Fraction:
    return k * u / (1 - k * u)


def check_variance_against_fractions(T, defect=None):
    """The restated variance against the variance of the same rounded inputs in exact rational arithmetic.

    The bound.  u = 2^-24 (float32) or 2^-53 (float64), gamma_k = k u / (1 - k u); the n valid entries have weights w_j >= 0, D = sum w,
    N = sum w x, mu = N / D, V = sum w (x - mu)^2 / D, A = sum w |x| / D; no overflow, no underflow (rows that hold an infinity or a
    subnormal are left out).
      * num = fl(sum fl(w x)) in sequence: one rounding per product and n - 1 per sum, |num - N| <= gamma_n A D.
      * den = D (1 + theta), |theta| <= gamma_{n-1}: a sequential sum of non-negative terms.
      * mean = fl(num / den) = (num / D) (1 + phi), |phi| <= gamma_n (n - 1 roundings of den, one of the division), so
        |mean - mu| <= gamma_n |mu| + gamma_n A (1 + gamma_n) <= e_m := gamma_n A (2 + gamma_n)              (|mu| <= A).
      * each term fl(w fl(fl(x - mean)^2)) carries 2 + 1 + 1 roundings, the sequential sum n - 1, the last division by den another
        n - 1 + 1: s / den = (S(mean) / D) (1 + eta), |eta| <= gamma_{2n+3}, where S(m) = sum w (x - m)^2 — every term is non-negative,
        so the relative errors carry over to the sum.
      * S(m) / D = V + (m - mu)^2 exactly.
    Hence |out - V| <= gamma_{2n+3} (V + e_m^2) + e_m^2.  Checked in rational arithmetic, so the bound itself is not rounded."""
    u = Fraction(1, 2**24) if T is np.float32 else Fraction(1, 2**53)
    case = bs.make_case(T, 3)
    got = bs.restate(case, bs.VARIANCE, bs.ALL, 0.0, defect)
    root = bs.restate(case, bs.STDDEV, bs.ALL, 0.0, defect)
    tiny = np.finfo(T).tiny
    checked = 0
    for t, idx, w in rows_of(case):
        for l in range(case.n_lev):
            x = case.src[idx, l]
            keep = ~np.isnan(x)
            if not keep.any():
                assert np.isnan(got[t, l])
                continue
            xs, ws = x[keep], w[keep]
            with np.errstate(all="ignore"):  # numpy's sqrt rounds correctly
                assert root.dtype == got.dtype and bs.same(root[t, l: l + 1], np.sqrt(got[t, l: l + 1])).all()
            if not np.isfinite(xs).all() or ((xs != 0) & (np.abs(xs) < tiny)).any() or not (ws.astype(np.float64).sum() > 0):
                continue  # (inf - inf, or 0 / 0 where the only valid weight is 0: whatever the arithmetic gives)
            assert got[t, l] == got[t, l]
            n = len(xs)
            fx, fw = [Fraction(float(v)) for v in xs], [Fraction(float(v)) for v in ws]
            D = sum(fw)
            mu = sum(a * b for a, b in zip(fw, fx)) / D
            V = sum(a * (b - mu) ** 2 for a, b in zip(fw, fx)) / D
            A = sum(a * abs(b) for a, b in zip(fw, fx)) / D
            e_m = gamma(n, u) * A * (2 + gamma(n, u))
            bound = gamma(2 * n + 3, u) * (V + e_m**2) + e_m**2
            assert abs(Fraction(float(got[t, l])) - V) <= bound, (t, l, n, float(got[t, l]), float(V), float(bound))
            checked += 1
    assert checked > 200


def as_missing_case(case: bs.StatCase) -> ms.MissingCase:
    lengths = np.diff(case.indptr)
    k = int(lengths.max())
    present = np.arange(k)[None, :] < lengths[:, None]
    idx, w = np.full((case.n_tgt, k), -1, dtype=np.int32), np.zeros((case.n_tgt, k), dtype=case.T)
    idx[present], w[present] = case.indices, case.data
    return ms.MissingCase("from-" + case.name, case.T, k, case.n_lev, case.n_src, case.n_tgt, idx, w, case.src)


def check_nan_pattern_against_the_missing_value_restatement(T, defect=None):
    """The same tables, the same policy: the targets this statement makes NaN under ALL / HEAVIEST are those the gather's statement
    (tests/regrid_missing_restatement.py) makes NaN by a policy branch — empty rows aside, which the gather gives 0."""
    case = bs.make_case(T, 6)
    filled = np.diff(case.indptr) > 0
    for policy, min_valid in ((bs.ALL, 0.0), (bs.HEAVIEST, 0.0), (bs.ALL, 0.5), (bs.HEAVIEST, 1.0), (bs.ALL, 1.0)):
        _, branch = ms.restate(as_missing_case(case), policy, min_valid)
        gone = np.isin(branch, (ms.ALL_MISSING, ms.HEAVIEST_MISSING, ms.BELOW_MIN_VALID))
        got = bs.restate(case, bs.MINIMUM, policy, min_valid, defect)
        assert np.array_equal(np.isnan(got)[filled], gone[filled]), (policy, min_valid)
        assert np.isnan(got[~filled]).all()
        assert 0 < gone[filled].sum() < gone[filled].size
    # ANY: NaN exactly where a source is NaN (or the row is empty)
    got = bs.restate(case, bs.MAXIMUM, bs.ANY, 0.0, defect)
    for t, idx, _ in rows_of(case):
        assert np.array_equal(np.isnan(got[t]), np.isnan(case.src[idx]).any(axis=0) | (len(idx) == 0))


CHECKS = (check_extremes_against_reduceat, check_mode_against_classes, check_variance_against_fractions,
          check_nan_pattern_against_the_missing_value_restatement)


@pytest.mark.parametrize("T", WIDTHS)
@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__)
def test_the_restatement_agrees_with_an_independent_route(check, T):
    check(T)


@pytest.mark.parametrize("defect", bs.DEFECTS)
def test_the_routes_catch_a_planted_defect(defect):
    caught = []
    for check in CHECKS:
        try:
            check(np.float64, defect)
        except AssertionError:
            caught.append(check.__name__)
    assert caught, f"no independent route notices {defect}"


def test_mode_edge_rows_of_the_restatement():
    T = np.float64
    inf = np.inf
    case = bs.rows_case(T, "mode-edges", [[4, 4, 4], [1, 2, 3], [3, 1], [-0.0, 0.0, 5], [0.0, -0.0, 5], [np.nan, 2, np.nan, 2, 7], [inf, -inf, inf], []],
                        [[0.25] * 3, [0.25] * 3, [0.25] * 2, [0.25, 0.25, 0.25], [0.25, 0.25, 0.25], [0.5, 0.125, 0.5, 0.125, 0.125], [0.25] * 3, []])
    got = bs.restate(case, bs.MODE, bs.ALL, 0.0)[:, 0]
    assert got[:3].tolist() == [4.0, 1.0, 1.0] and got[5] == 2.0 and got[6] == inf and np.isnan(got[7])
    assert got[3] == 0 and np.signbit(got[3]) and got[4] == 0 and not np.signbit(got[4])  # one class; the first one met is written
    assert np.isnan(bs.restate(case, bs.MODE, bs.ANY, 0.0)[5, 0]) and np.isnan(bs.restate(case, bs.MODE, bs.HEAVIEST, 0.0)[5, 0])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_agree():
    import abi_checks

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "atx_stat.h")
    declared = abi_checks.header_declarations(header, "ATX_STAT_API")
    assert declared == ["atx_stat_version", "atx_stat_last_error", "atx_regrid_csr_stat"]
    assert list(native_stat.SIGNATURES) == declared and not set(declared) & set(native.SIGNATURES)
    assert native_stat.load().atx_stat_version() == 420 and "#define ATX_STAT_VERSION 420" in open(header).read()
    if abi_checks.nm_tool():
        assert abi_checks.defined_dynamic_symbols(native_stat.lib_path())[0] == sorted(declared)


def source_text() -> str:
    return open(os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc", "stat", "atx_regrid_stat.hip")).read()


def test_no_kernel_uses_scratch_memory_or_lds():
    """Read from the code objects inside libatx_stat.so (tools/kernel_resources.py; no GPU)."""
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernel_resources(native_stat.lib_path())
    kernels = [r for r in rows if "stat_kernel" in r["name"]]
    assert len(kernels) == 24  # 2 widths x (vector, scalar) x (maximum, minimum: with and without weights; mode; variance)
    assert [r["name"] for r in rows if r["scratch"] > 0 or r["lds"] > 0] == []


def test_abi_argument_validation_without_a_gpu():
    """Bad arguments are refused before anything touches HIP, with the status codes of atx_regrid_csr_missing and a message each."""
    lib = native_stat.load()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    fn = lib.atx_regrid_csr_stat

    def call(src=one, out=one, indptr=one, indices=one, data=one, n_src=8, n_tgt=8, nnz=8, n_lev=4, sp=4, op=4, dtype=0, layout=0, statistic=0,
             policy=0, min_valid=0.0):
        return fn(src, out, indptr, indices, data, n_src, n_tgt, nnz, n_lev, sp, op, dtype, layout, statistic, policy, min_valid, None)

    def said() -> str:
        return lib.atx_stat_last_error().decode()

    assert call(src=None) == native.EINVAL and said() == "atx_regrid_csr_stat: null src/out pointer"
    assert call(out=None) == native.EINVAL and call(indptr=None) == native.EINVAL and said() == "atx_regrid_csr_stat: null indptr"
    assert call(indices=None) == native.EINVAL and said() == "atx_regrid_csr_stat: null indices"
    assert call(dtype=7) == native.EINVAL and call(layout=5) == native.EINVAL and call(n_lev=0) == native.EINVAL
    assert call(sp=3) == native.ESHAPE and call(op=3) == native.ESHAPE and call(nnz=-1) == native.ENOTIMPL
    for bad in (-1, 5, 99):
        assert call(statistic=bad) == native.EINVAL and said() == f"atx_regrid_csr_stat: unknown statistic {bad}"
    for bad in (-1, 3):
        assert call(policy=bad) == native.EINVAL and said() == f"atx_regrid_csr_stat: unknown missing-value policy {bad}"
    for bad, text in ((-0.1, "-0.1"), (1.5, "1.5"), (float("nan"), "nan")):
        assert call(min_valid=bad) == native.EINVAL and said() == f"atx_regrid_csr_stat: min_valid = {text} is outside [0, 1]"
    for statistic in (native_stat.MODE, native_stat.VARIANCE, native_stat.STDDEV):
        assert call(data=None, statistic=statistic) == native.EINVAL
        assert said() == "atx_regrid_csr_stat: null data (only the maximum and the minimum are defined without weights)"
    assert call(layout=1, sp=8, op=8) == native.ENOTIMPL
    assert said() == "atx_regrid_csr_stat: column stacks only (convert an ATX_FIELDS stack with atx_relayout)"
    # no targets: validated, nothing launched — with and without weights
    assert call(out=None, indptr=None, indices=None, data=None, nnz=0, n_tgt=0) == native.OK
    assert call(out=None, indptr=None, n_tgt=0, statistic=native_stat.MODE) == native.OK
    assert call(out=None, indptr=None, n_tgt=0, statistic=9) == native.EINVAL  # ... validated all the same
    with pytest.raises(RuntimeError, match="HBM-resident"):
        import torch

        native_stat.regrid_csr_stat(torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(5, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), None,
                                    n_src=4, n_tgt=4, nnz=4, n_lev=4, src_pitch=4, out_pitch=4, layout=native.COLUMNS, statistic="maximum")
    with pytest.raises(ValueError, match="statistic"):
        native_stat.statistic_code("median")
    with pytest.raises(ValueError, match="policy"):
        native_stat.missing_policy_code("some")
    assert [native_stat.statistic_code(s) for s in bs.STATISTICS] == [0, 1, 2, 3, 4]
    assert [native_stat.missing_policy_code(p) for p in (None, "all", "heaviest")] == [0, 1, 2]


def test_the_class_table_has_a_named_capacity():
    import re

    assert re.findall(r"constexpr int kModeClasses = (\d+);", source_text()) == ["8"]


# ---- the Python layers -------------------------------------------------------------------------------------------------------------
def tiny_matrix():
    lat, lon = np.array([10.0, 0.0, -10.0]), np.array([0.0, 10.0, 20.0])
    return dict(matrix_shape=np.array([3, 5]), matrix_data=np.array([0.5, 0.5, 0.25, 0.75, 1.0]), matrix_indices=np.array([0, 1, 1, 2, 4], dtype=np.int32),
                matrix_indptr=np.array([0, 2, 4, 5], dtype=np.int32), out_latitudes=lat, out_longitudes=lon)


def test_reduce_validates_its_arguments_before_it_touches_the_stack():
    plan = GatherPlan(5, 3, index=np.array([[0, 1], [1, 2], [3, 4]]), weights=np.full((3, 2), 0.5))
    with pytest.raises(ValueError, match="apply"):
        plan.reduce(None, "mean")
    with pytest.raises(ValueError, match="statistic.*maximum.*standard-deviation"):
        plan.reduce(None, "median")
    with pytest.raises(ValueError, match="missing="):
        plan.reduce(None, "maximum", missing="missing-if-all-missing")  # the filter's spellings are the filter's
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_valid"):
            plan.reduce(None, "maximum", min_valid=bad)
    copy = GatherPlan(5, 3, index=np.array([0, 2, 4]))
    for statistic in ("mode", "variance", "standard-deviation"):
        with pytest.raises(ValueError, match="needs weights"):
            copy.reduce(None, statistic)


def test_a_plans_rows_as_the_statistics_read_them():
    from anemoi_transform_amd.interp import ell_to_csr

    rng = np.random.default_rng(3)
    index, weights = rng.integers(0, 9, (6, 4)), rng.random((6, 4))
    plan = GatherPlan(9, 6, index=index, weights=weights)
    m = ell_to_csr(index, weights, 9)
    indptr, indices, data = plan._stat_rows()
    assert np.array_equal(indptr, m["matrix_indptr"]) and np.array_equal(indices, m["matrix_indices"]) and np.array_equal(data, m["matrix_data"])
    assert plan._stat_rows() is plan._stat_rows()  # converted once
    padded = GatherPlan(9, 3, index=np.array([[1, -1, 2], [-1, -1, -1], [4, 5, 6]]), weights=np.array([[0.5, 7.0, 0.5], [7.0] * 3, [0.25, 0.25, 0.5]]),
                        padded=True)
    indptr, indices, data = padded._stat_rows()
    assert indptr.tolist() == [0, 2, 2, 5] and indices.tolist() == [1, 2, 4, 5, 6] and data.tolist() == [0.5, 0.5, 0.25, 0.25, 0.5]
    assert indptr.dtype == np.int32 and indices.dtype == np.int32
    copy = GatherPlan(9, 3, index=np.array([0, 2, 4]))
    indptr, indices, data = copy._stat_rows()
    assert indptr.tolist() == [0, 1, 2, 3] and indices.tolist() == [0, 2, 4] and data is None
    csr = GatherPlan.from_matrix(dict(matrix_shape=np.array([3, 9]), matrix_data=np.arange(23.0), matrix_indices=np.arange(23) % 9,
                                      matrix_indptr=np.array([0, 20, 21, 23])))
    assert csr.kind == "csr" and csr._stat_rows()[0].tolist() == [0, 20, 21, 23] and csr._stat_rows()[1] is csr.indices


def test_filter_construction(caplog):
    from anemoi_transform_amd.core import reset_notes

    for statistic in ("maximum", "minimum", "mode", "variance", "standard-deviation"):
        f = create_filter_by_name("regrid", matrix=tiny_matrix(), statistic=statistic, missing="missing-if-all-missing", min_valid=0.25)
        assert f.statistic == statistic and f.missing == "all" and f.min_valid == 0.25
        assert fusion._gather_head(f) is None  # runs alone: the fused launch has no such kernel
    mean = create_filter_by_name("regrid", matrix=tiny_matrix(), statistic="mean")
    assert mean.statistic is None and fusion._gather_head(mean) is mean  # the gather itself, fusion included
    choices = "'maximum', 'minimum', 'mode', 'variance', 'standard-deviation', 'mean'"
    for bad in ("median", "max", "", 1):
        with pytest.raises(ValueError, match=choices):
            create_filter_by_name("regrid", matrix=tiny_matrix(), statistic=bad)
    with pytest.raises(ValueError, match=choices):
        create_filter_by_name("regrid", in_grid="O16", out_grid="O4", method="grid-box-statistics")
    for config in (dict(in_grid="O16", out_grid="O4", method="nearest"), dict(mask=np.array([0, 2])), dict(in_grid="O16", out_grid="O4", method="linear"),
                   dict(in_grid="O16", out_grid="O4", method="grid-box-average"), dict(in_grid="O16", out_grid="O4")):
        with pytest.raises(ValueError, match=choices):
            create_filter_by_name("regrid", statistic="maximum", **config)
    # the grids obey the rules of grid-box-average: the same NotImplementedError, pointing at matrix=
    unstructured = dict(latitudes=np.array([10.0, 0.0, -10.0]), longitudes=np.array([0.0, 10.0, 20.0]))
    for grids in (dict(in_grid="O16", out_grid=unstructured), dict(in_grid=unstructured, out_grid="O4")):
        with pytest.raises(NotImplementedError) as stat:
            create_filter_by_name("regrid", method="grid-box-statistics", statistic="maximum", **grids)
        with pytest.raises(NotImplementedError) as mean:
            create_filter_by_name("regrid", method="grid-box-average", **grids)
        assert "matrix" in str(stat.value) and str(stat.value) == str(mean.value).replace("grid-box-average", "grid-box-statistics")

    def notes(fresh, **config):
        if fresh:
            reset_notes()
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger="anemoi_transform_amd"):
            create_filter_by_name("regrid", matrix=tiny_matrix(), **config)
        return [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING and "unpinned" in r.getMessage()]

    said = notes(True, statistic="mode")
    assert len(said) == 1 and "MIR" in said[0] and "in-tree" in said[0] and "include/atx_stat.h" in said[0]
    assert notes(False, statistic="maximum") == []  # once per process
    said = notes(True, statistic="variance", missing="missing-if-all-missing")  # the policy is part of the same statement: one note
    assert len(said) == 1 and "include/atx_stat.h" in said[0]
    assert notes(True, statistic="mean") == [] and notes(True) == []  # the gather has nothing new to say


def test_the_mean_builds_the_plan_of_grid_box_average():
    a = create_filter_by_name("regrid", in_grid="O16", out_grid="O4", method="grid-box-statistics", statistic="mean").interpolator.plan
    b = create_filter_by_name("regrid", in_grid="O16", out_grid="O4", method="grid-box-average").interpolator.plan
    c = create_filter_by_name("regrid", in_grid="O16", out_grid="O4", method="grid-box-statistics", statistic="maximum").interpolator.plan
    for plan in (a, c):
        assert (plan.kind, plan.n_src, plan.n_tgt, plan.k, plan.padded) == (b.kind, b.n_src, b.n_tgt, b.k, b.padded)
        if b.kind == "csr":
            assert np.array_equal(plan.indptr, b.indptr) and np.array_equal(plan.indices, b.indices) and np.array_equal(plan.data, b.data)
        else:
            assert np.array_equal(plan.index, b.index) and np.array_equal(plan.weights, b.weights)
