"""Model levels to pressure levels without a GPU: the restatement of include/atx_levels.h (tests/levels_restatement.py) against exact
arithmetic and ``np.interp``, once as it is and once per planted defect through the comparisons the GPU test uses; then the C ABI's
argument validation through ctypes, the kernels' resources, and the errors of the ``ml_to_pl`` filter.

The bounds of ``test_the_restatement_is_close_to_exact_arithmetic`` are derived, not measured.  u = 2^-53; every A[j], B[j] sp >= 0 in
the cases here, so p_half carries two roundings and p_full a third without cancellation: |d p_full| <= 3 u p_full.  With D = c(p_b) -
c(p_a) exact and w in [0, 1]:
  linear  |dw| <= u (9 p_b / D + 3): the numerator carries |d p_a| and one rounding, the denominator |d p_a| + |d p_b| and one rounding,
          the division one more;
  log     a logarithm within 1 ulp of a pressure within 3 u: |d c| <= u (|c| + 3), so |dw| <= u ((4 L + 9) / D + 3), L the largest |c|.
y = x_a + w (x_b - x_a) adds the roundings of the difference, the product and the sum: with M = max(|x_a|, |x_b|), |x_b - x_a| <= 2 M and
one ulp of M >= u M, the distance from exact is at most 2 (|dw| / u + 2) + 1 ulps of M — and one rounding more, 0.5, for a float32 stack,
whose float64 arithmetic counts 2^-29 as much.
"""

from __future__ import annotations

import ctypes
import functools
import json
import logging
import math
import os

import numpy as np
import pytest

from anemoi_transform_amd import native, native_levels
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.core import filter_registry

import levels_restatement as lr
from hybrid_column_common import WIDTHS, fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULPS_FILE = os.path.join(ROOT, "profiles", "levels_ulps.json")


# ---- the restatement against exact arithmetic -------------------------------------------------------------------------------------
def derived_bounds(case: lr.LevelsCase, coordinate) -> np.ndarray:
    """The module docstring's bound per (point, target) in ulps of max(|x[a]|, |x[b]|) of the case's type (NaN: not interior)."""
    out = np.full((case.n_pts, case.n_tgt), np.nan)
    for p in range(case.n_pts):
        pf, ground, s = lr.full_levels(case, p)
        for t in range(case.n_tgt):
            kind, a, b, _ = lr.bracket(pf, ground, s, case.targets[t], lr.LINEAR, lr.NEAREST)
            if kind != lr.INTERIOR:
                continue
            pa, pb, P = float(pf[a]), float(pf[b]), float(case.targets[t])
            if coordinate == lr.LOG:
                L = max(abs(math.log(pa)), abs(math.log(pb)), abs(math.log(P)))
                dw = (4 * L + 9) / (math.log(pb) - math.log(pa)) + 3
            else:
                dw = 9 * pb / (pb - pa) + 3
            f64 = 2 * (dw + 2) + 1
            out[p, t] = f64 if case.T is np.float64 else 0.5 + f64 * 2.0**-29
    return out


@functools.lru_cache(maxsize=None)
def restatement_errors(T, coordinate):
    case = lr.base_case(T, specials=False)
    value, unit = lr.exact_reference(case, coordinate)
    e = lr.errors(lr.reference(case, coordinate, lr.NEAREST), value, unit)
    return case, e


@pytest.mark.parametrize("coordinate", [lr.LINEAR, lr.LOG])
@pytest.mark.parametrize("T", WIDTHS)
def test_the_restatement_is_close_to_exact_arithmetic(T, coordinate):
    case, e = restatement_errors(T, coordinate)
    bound = np.broadcast_to(derived_bounds(case, coordinate)[:, None, :], e.shape)
    checked = ~np.isnan(e)
    assert checked.sum() > 0.25 * e.size and np.array_equal(checked, ~np.isnan(bound))  # every interior element has an exact value
    assert (e[checked] <= bound[checked]).all(), (float(e[checked].max()), np.argwhere(checked & (e > bound))[:5].tolist())


def test_the_largest_distance_from_exact_is_on_record():
    """profiles/levels_ulps.json, section "restatement": numpy's float64 arithmetic on the base case, in ulps of max(|x[a]|, |x[b]|).
    The section "kernel" is the GPU test's (tests/test_gpu_levels.py prints it); this test leaves it as it is."""
    record = {}
    for T in (np.float32, np.float64):
        for coordinate in (lr.LINEAR, lr.LOG):
            _, e = restatement_errors(T, coordinate)
            record[f"{np.dtype(T).name}-{coordinate}"] = round(float(np.nanmax(e)), 4)
    on_file = json.load(open(ULPS_FILE)) if os.path.exists(ULPS_FILE) else {}
    if on_file.get("restatement") != record:
        on_file.update(unit="ulps of max(|x[a]|, |x[b]|) in the stack's type", case="base case of tests/levels_restatement.py, finite columns",
                       restatement=record)
        with open(ULPS_FILE, "w") as f:
            json.dump(on_file, f, indent=1)
            f.write("\n")
    assert json.load(open(ULPS_FILE))["restatement"] == record
    assert record["float32-linear"] <= 0.5 + 1e-3 and record["float32-log"] <= 0.5 + 1e-3  # one rounding


@pytest.mark.parametrize("coordinate", [lr.LINEAR, lr.LOG])
@pytest.mark.parametrize("T", WIDTHS)
def test_a_target_on_a_full_level_returns_the_levels_bits(T, coordinate):
    case = lr.base_case(T, specials=False)
    on_level = lr.on_a_full_level(case)
    assert on_level.sum() >= 5
    got = lr.reference(case, coordinate, lr.MISSING)
    seen = 0
    for p, t in np.argwhere(on_level):
        pf = lr.full_levels(case, p)[0]
        k = [float(v) for v in pf].index(float(case.targets[t]))
        assert np.array_equal(got[p, :, t].view(lr.bits_type(T)), case.x[p, :, k].view(lr.bits_type(T))), (p, t, k)
        seen += 1
    assert seen >= 5


@pytest.mark.parametrize("coordinate", [lr.LINEAR, lr.LOG])
def test_fields_affine_in_the_coordinate_come_back_affine(coordinate):
    case = lr.base_case(np.float64, specials=False)
    c = (lambda p: p) if coordinate == lr.LINEAR else np.log
    alpha, beta = 3.0, -0.25
    x = np.empty((case.n_pts, 1, case.n_lev))
    for p in range(case.n_pts):
        x[p, 0] = alpha + beta * c(np.array(lr.full_levels(case, p)[0]))
    affine = lr.LevelsCase("affine", np.float64, case.A, case.B, None, case.sp, x, case.targets)
    got = lr.restate(affine, coordinate, lr.MISSING)[:, 0, :]
    interior = lr.classes(affine) == lr.INTERIOR
    want = alpha + beta * c(np.broadcast_to(case.targets, got.shape))
    assert interior.sum() > 1000 and np.allclose(got[interior], want[interior], rtol=1e-12, atol=0.0)
    assert np.isnan(got[(lr.classes(affine) == lr.ABOVE_TOP) | (lr.classes(affine) == lr.BELOW_GROUND)]).all()


def test_np_interp_agrees_on_monotone_columns():
    """np.interp clamps at both ends: the "nearest" policy, and the lowest level's value in the half layer above the ground."""
    case = lr.base_case(np.float64, specials=False)
    got = lr.reference(case, lr.LINEAR, lr.NEAREST)
    for p in range(case.n_pts):
        pf = np.array(lr.full_levels(case, p)[0])
        assert (np.diff(pf) > 0).all()
        for v in range(case.n_var):
            assert np.allclose(got[p, v], np.interp(case.targets, pf, case.x[p, v]))


def test_the_base_case_reaches_every_class():
    shares = lr.base_class_shares(np.float64)
    assert shares[lr.INTERIOR] >= 0.25 and all(shares[c] > 0 for c in lr.CLASSES), shares
    assert abs(sum(shares.values()) - 1.0) < 1e-12


# ---- planted defects ---------------------------------------------------------------------------------------------------------------
def test_the_restatement_passes_its_own_comparisons():
    lr.check_linear(lambda case, c, o: lr.restate(case, c, o), lr.edge_cases(np.float64))
    lr.check_log(lambda case, c, o: lr.restate(case, c, o), lr.edge_cases(np.float64)[:1])


@pytest.mark.parametrize("defect", lr.DEFECTS)
def test_the_comparisons_catch_a_planted_defect(defect):
    """Each wrong reading of the statement, planted in a copy of the restatement, fails a comparison the GPU test makes."""
    caught = []
    for check, cases in ((lr.check_linear, lr.edge_cases(np.float64)), (lr.check_log, lr.edge_cases(np.float64)[:1])):
        try:
            check(lambda case, c, o: lr.restate(case, c, o, defect=defect), cases)
        except AssertionError:
            caught.append(check.__name__)
    assert caught, f"no comparison notices {defect}"
    if defect == "weight-in-p":
        assert caught == ["check_log"]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_agree():
    import abi_checks

    header = os.path.join(ROOT, "include", "atx_levels.h")
    declared = abi_checks.header_declarations(header, "ATX_LEVELS_API")
    assert declared == ["atx_levels_version", "atx_levels_last_error", "atx_levels_interpolate"]
    assert list(native_levels.SIGNATURES) == declared and not set(declared) & set(native.SIGNATURES)
    assert native_levels.load().atx_levels_version() == 420 and "#define ATX_LEVELS_VERSION 420" in open(header).read()
    assert f"#define ATX_LEVELS_MAX_LEVELS {native_levels.MAX_LEVELS}" in open(header).read()
    if abi_checks.nm_tool():
        assert abi_checks.defined_dynamic_symbols(native_levels.lib_path())[0] == sorted(declared)
    import __graft_entry__ as graft

    assert [lib.binding for lib in graft.LIBRARIES].count("native_levels") == 1


def test_no_kernel_uses_scratch_memory():
    """Read from the code objects inside libatx_levels.so (tools/kernel_resources.py; no GPU).  The LDS of the column kernels is asked
    for at the launch (the tile is sized by the shape), so the fixed size is zero for every kernel."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernel_resources(native_levels.lib_path())
    assert len([r for r in rows if "levels_columns_kernel" in r["name"]]) == 8  # 2 widths x (vector, scalar) x (linear, log)
    assert len([r for r in rows if "levels_fields_kernel" in r["name"]]) == 4  # 2 widths x (linear, log)
    assert len(rows) == 12 and [r["name"] for r in rows if r["scratch"] > 0 or r["lds"] > 0] == []
    record = json.load(open(os.path.join(ROOT, "profiles", "levels_resources.json")))
    assert record["library"].endswith("libatx_levels.so") and len(record["kernels"]) == 12 and all(k["scratch"] == 0 for k in record["kernels"])


def test_abi_argument_validation_without_a_gpu():
    """Every refusal of include/atx_levels.h comes before anything touches HIP: the device pointers are never dereferenced."""
    lib = native_levels.load()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    fn = lib.atx_levels_interpolate

    def call(src=one, out=one, sp=one, A=one, B=one, index=None, targets=one, n_pts=8, n_var=1, n_lev=4, n_tgt=3, n_half=5, src_pitch=4, out_pitch=3,
             dtype=0, layout=0, coordinate=0, outside=0):
        if index is not None:
            index = (ctypes.c_int32 * len(index))(*index)
        return fn(src, out, sp, A, B, index, targets, n_pts, n_var, n_lev, n_tgt, n_half, src_pitch, out_pitch, dtype, layout, coordinate, outside, None)

    def said() -> str:
        return lib.atx_levels_last_error().decode()

    name = "atx_levels_interpolate"
    # null pointers of non-empty buffers
    for arg in ("src", "sp"):
        assert call(**{arg: None}) == native.EINVAL and said() == f"{name}: null src / sp pointer"
    assert call(out=None) == native.EINVAL and said() == f"{name}: null out pointer"
    assert call(targets=None) == native.EINVAL and said() == f"{name}: null targets"
    for arg in ("A", "B"):
        assert call(**{arg: None}) == native.EINVAL and said() == f"{name}: null A / B coefficients"
    # sizes
    assert call(n_lev=0) == native.EINVAL and "bad sizes" in said()
    assert call(n_var=0) == native.EINVAL and call(n_pts=-1) == native.EINVAL and call(n_tgt=-1) == native.EINVAL
    for bad in (1, 0, -3):
        assert call(n_half=bad) == native.EINVAL and said() == f"{name}: n_half={bad}: a model has at least one level, two half levels"
    # pitches too small for the shape, in both layouts
    assert call(src_pitch=3) == native.ESHAPE and "column pitch (3, 3) < rows (4, 3)" in said()
    assert call(out_pitch=2) == native.ESHAPE and call(n_var=2, src_pitch=7, out_pitch=6) == native.ESHAPE
    assert call(n_var=2, src_pitch=8, out_pitch=5) == native.ESHAPE
    assert call(layout=1, src_pitch=7, out_pitch=8) == native.ESHAPE and "field pitch (7, 8) < points 8" in said()
    assert call(layout=1, src_pitch=8, out_pitch=7) == native.ESHAPE
    # the level index: strictly increasing inside 0 .. n_half - 2; without one, the rows are levels 0 .. n_lev - 1 of the table
    assert call(n_half=4) == native.EINVAL and said() == f"{name}: n_lev=4 rows without a level_index need n_half >= 5, got 4"
    for bad, k in (([0, 1, 1, 2], 2), ([0, 2, 1, 3], 2), ([-1, 0, 1, 2], 0), ([0, 1, 2, 4], 3), ([3, 2, 1, 0], 1)):
        assert call(index=bad) == native.EINVAL
        assert said() == f"{name}: level_index[{k}] = {bad[k]} is not strictly increasing inside 0 .. 3"
    assert call(index=[0, 1, 2, 9], n_half=10) == native.EINVAL and said() == f"{name}: level_index[3] = 9 is not strictly increasing inside 0 .. 8"
    assert call(index=[0, 1, 2, 8], n_half=10, n_tgt=0, out_pitch=0) == native.OK  # the lowest model level of a longer table (no targets: no launch)
    # unknown codes
    assert call(dtype=7) == native.EINVAL and said() == f"{name}: bad dtype 7"
    assert call(layout=5) == native.EINVAL and said() == f"{name}: bad layout 5"
    for bad in (-1, 2):
        assert call(coordinate=bad) == native.EINVAL and said() == f"{name}: unknown coordinate {bad}"
        assert call(outside=bad) == native.EINVAL and said() == f"{name}: unknown outside policy {bad}"
    # beyond a stated limit: not implemented, never a silently wrong result
    assert call(n_lev=257, n_half=258, src_pitch=257) == native.ENOTIMPL and "exceeds the 256 levels of one call" in said()
    assert call(n_pts=2**31, layout=0) == native.ENOTIMPL and call(n_tgt=65536, out_pitch=65536) == native.ENOTIMPL
    assert call(n_var=300, n_lev=250, n_half=251, src_pitch=75000) == native.ENOTIMPL
    # no points or no targets: validated, nothing launched
    assert call(src=None, out=None, sp=None, n_pts=0) == native.OK and call(out=None, targets=None, n_tgt=0, out_pitch=0) == native.OK
    assert call(src=None, out=None, sp=None, n_pts=0, coordinate=9) == native.EINVAL  # ... validated all the same
    assert call(index=[1, 2, 3, 4], n_half=6, src=None, out=None, sp=None, n_pts=0) == native.OK  # a subset of a longer table
    # the Python binding
    import torch

    with pytest.raises(RuntimeError, match="HBM-resident"):
        native_levels.interpolate(torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4), torch.zeros(5, dtype=torch.float64),
                                  torch.zeros(5, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), n_pts=4, n_var=1, n_lev=4, n_tgt=3, src_pitch=4,
                                  out_pitch=4, layout=native.COLUMNS)
    with pytest.raises(ValueError, match="coordinate"):
        native_levels.coordinate_code("cubic")
    with pytest.raises(ValueError, match="outside"):
        native_levels.outside_code("extrapolate")
    assert [native_levels.coordinate_code(c) for c in ("linear", "log")] == [0, 1]
    assert [native_levels.outside_code(o) for o in ("nearest", "missing")] == [0, 1]


# ---- the filter --------------------------------------------------------------------------------------------------------------------
AB = dict(A=[0.0, 2000.0, 4000.0, 0.0], B=[0.0, 0.1, 0.5, 1.0])  # three model levels


def test_the_filter_is_registered_and_checks_its_configuration():
    assert "ml_to_pl" in filter_registry.registered
    f = create_filter_by_name("ml_to_pl", levels=[1000, 850.5, 500], model_level_AB=AB)
    assert f.levels == [1000, 850.5, 500] and f.targets_pa == [100000.0, 85050.0, 50000.0] and isinstance(f.levels[0], int)
    assert (f.interpolation, f.outside, f.surface_pressure, f.params) == ("linear", "nearest", "sp", None)
    for bad in ([], [1000, 1000], [0], [-5], ["high"], [float("nan")]):
        with pytest.raises(ValueError, match="levels"):
            create_filter_by_name("ml_to_pl", levels=bad, model_level_AB=AB)
    with pytest.raises(ValueError, match="interpolation must be one of 'linear', 'log'"):
        create_filter_by_name("ml_to_pl", levels=[500], model_level_AB=AB, interpolation="cubic")
    with pytest.raises(ValueError, match="outside must be one of 'nearest', 'missing'"):
        create_filter_by_name("ml_to_pl", levels=[500], model_level_AB=AB, outside="extrapolate")
    with pytest.raises(ValueError, match="same length"):
        create_filter_by_name("ml_to_pl", levels=[500], model_level_AB=dict(A=[0.0, 1.0], B=[0.0, 0.5, 1.0]))
    # model_level_AB is handled by filters/domain.py: the same errors, the same registry of names
    with pytest.raises(KeyError, match="predefined AB-coefficients"):
        create_filter_by_name("ml_to_pl", levels=[500], model_level_AB="IFS_137")
    with pytest.raises(TypeError, match="string or a dictionary"):
        create_filter_by_name("ml_to_pl", levels=[500], model_level_AB=[1, 2])
    from anemoi_transform_amd.filters import domain, vertical

    assert vertical._set_AB is domain._set_AB
    domain.register_model_level_AB("three_levels_for_ml_to_pl", AB["A"], AB["B"])
    try:
        named = create_filter_by_name("ml_to_pl", levels=[500], model_level_AB="three_levels_for_ml_to_pl")
        assert named.A.tolist() == AB["A"] and named.B.tolist() == AB["B"]
    finally:
        del domain.MODEL_LEVEL_AB["THREE_LEVELS_FOR_ML_TO_PL"]


def test_grouping_errors_come_before_any_launch():
    """Host fields, no GPU here: each of these raises from the bookkeeping, before a stack is built or a kernel launched."""
    f = create_filter_by_name("ml_to_pl", levels=[850, 500], model_level_AB=AB)
    ml = [("t", "ml", 1), ("t", "ml", 2), ("t", "ml", 3)]
    with pytest.raises(ValueError, match="no surface pressure 'sp'") as no_sp:
        f.forward(fields(*ml))
    assert "lnsp" not in str(no_sp.value)
    with pytest.raises(ValueError, match=r"no surface pressure 'sp'.*lnsp_to_sp \| ml_to_pl"):
        f.forward(fields(*ml, ("lnsp", "ml", 1)))
    with pytest.raises(ValueError, match="Duplicate component t .* level 2"):
        f.forward(fields(*ml, ("t", "ml", 2), ("sp", "sfc", None)))
    with pytest.raises(ValueError, match="level 4 of t is outside the 3 model levels"):
        f.forward(fields(("t", "ml", 4), ("sp", "sfc", None)))
    with pytest.raises(ValueError, match="level 0 of q is outside"):
        f.forward(fields(("q", "ml", 0), ("sp", "sfc", None)))
    two_dates = list(fields(*ml, ("sp", "sfc", None))) + list(fields(("t", "ml", 2), ("t", "ml", 3), ("sp", "sfc", None), date=20260102))
    with pytest.raises(ValueError, match=r"mixed level sets for t: \[1, 2, 3\] and \[2, 3\]"):
        f.forward(two_dates)
    with pytest.raises(ValueError, match="Duplicate component sp"):
        f.forward(fields(*ml, ("sp", "sfc", None), ("sp", "sfc", None)))
    # the plan of a good list: what passes through, in input order, and what is interpolated, top first
    only_t = create_filter_by_name("ml_to_pl", levels=[500], model_level_AB=AB, params=["t"])
    data = fields(("q", "ml", 2), ("t", "ml", 3), ("sp", "sfc", None), ("t", "ml", 1), ("2t", "sfc", None), ("t", "pl", 500), ("t", "ml", 2), ("q", "ml", 1))
    passed, plan = only_t._plan(list(data))
    assert [(g.metadata("param"), g.metadata("levtype")) for g in passed] == [("q", "ml"), ("sp", "sfc"), ("2t", "sfc"), ("t", "pl"), ("q", "ml")]
    (sp, by_param), = plan
    assert sp.metadata("param") == "sp" and list(by_param) == ["t"] and [level for level, _ in by_param["t"]] == [3, 1, 2]
    passed, plan = f._plan(list(data))
    assert [g.metadata("param") for g in passed] == ["sp", "2t", "t"] and list(plan[0][1]) == ["q", "t"]


def test_the_unpinned_note_is_said_once(caplog):
    from anemoi_transform_amd.core import reset_notes

    def notes(fresh):
        if fresh:
            reset_notes()
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger="anemoi_transform_amd"):
            create_filter_by_name("ml_to_pl", levels=[500], model_level_AB=AB)
        return [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING and "unpinned" in r.getMessage()]

    said = notes(True)
    assert len(said) == 1 and "in-tree" in said[0] and "include/atx_levels.h" in said[0] and "earthkit-meteo" in said[0] and "MARS" in said[0]
    assert notes(False) == []  # once per process
    assert any("unpinned" in r.getMessage() and r.levelno == logging.DEBUG for r in caplog.records)  # still there for who asks


def test_interpolate_levels_checks_the_table_on_the_host():
    """A whole-model stack wants n_lev + 1 half levels (the assertion of filters/domain.py's _check_consistency); a subset says which."""
    import torch

    from anemoi_transform_amd.stack import Stack
    from anemoi_transform_amd.vertical import interpolate_levels

    stack = Stack(torch.zeros(4, 4), 4, 4, native.COLUMNS)
    with pytest.raises(AssertionError, match="one more vertical level"):
        interpolate_levels(stack, torch.zeros(4), np.zeros(7), np.zeros(7), [50000.0])
    with pytest.raises(AssertionError, match="same shape"):
        interpolate_levels(stack, torch.zeros(4), np.zeros(5), np.zeros(6), [50000.0])
    with pytest.raises(ValueError, match="3 variables"):
        interpolate_levels(stack, torch.zeros(4), np.zeros(5), np.zeros(5), [50000.0], n_var=3)
    with pytest.raises(ValueError, match="coordinate"):
        interpolate_levels(stack, torch.zeros(4), np.zeros(5), np.zeros(5), [50000.0], coordinate="cubic")
