"""Model levels to height levels without a GPU: the restatement of include/atx_heights.h (tests/heights_restatement.py) against exact
arithmetic, once as it is and once per planted defect through the comparison the GPU test uses; the conditions its cases must meet, in
exact arithmetic; numpy's own worst error per class, pinned; then the C ABI's argument validation through ctypes, the kernels'
resources, the host checks of ``vertical.interpolate_to_heights`` and the errors of the ``ml_to_hl`` filter.
"""

from __future__ import annotations

import ctypes
import json
import logging
import os

import numpy as np
import pytest

from anemoi_transform_amd import native, native_geopotential, native_heights, native_levels
from anemoi_transform_amd.core import filter_registry
from anemoi_transform_amd.filters import create_filter_by_name

import geopotential_restatement as gr
import heights_restatement as hr
from hybrid_column_common import fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# numpy's float64 arithmetic (the restatement before its rounding) against the exact statement on the float64 case of the class, in ulps
# of max(|x[a]|, |x[b]|): what the kernel's bounds (tests/test_gpu_heights.py) are relative to.  Measured here on the CPU, never from the
# kernel.  The error of c (tests/test_geopotential_host.py: the conditioning of alpha in thin layers) is divided by the thickness of the
# bracketing layer, which is what makes the figures of the long columns large; one level alone has no interior.
NUMPY_WORST_HEIGHTS = {
    (1, hr.WHOLE, hr.SEA): 0.0,
    (2, hr.SUBSET, hr.GROUND): 6.00,
    (3, hr.WHOLE, hr.SEA): 0.80,
    (17, hr.SUBSET, hr.GROUND): 30.98,
    (60, hr.WHOLE, hr.SEA): 213.58,
    (137, hr.WHOLE, hr.GROUND): 1833.94,
    (137, hr.SUBSET, hr.SEA): 1596.52,
}
CLASS_SHAPES = [shape for shape in hr.SHAPES if shape[0] > 0]


def shape_id(shape) -> str:
    return "-".join(str(v) for v in shape)


# ---- numpy's own error, pinned ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CLASS_SHAPES, ids=shape_id)
def test_numpy_worst_error_is_pinned(shape):
    case = hr.make_case(np.float64, *shape)
    worst, pinned = hr.numpy_worst(case), NUMPY_WORST_HEIGHTS[(case.n_lev, case.kind, case.reference)]
    print(f"heights {case.name}: numpy {worst:.4f} ulps of max(|x[a]|, |x[b]|)")
    assert 0.8 * pinned <= worst <= 1.1 * pinned + 0.1, (shape, worst, pinned)
    assert set(NUMPY_WORST_HEIGHTS) == {(n_lev, kind, reference) for n_pts, n_lev, kind, _, _, reference in CLASS_SHAPES}


@pytest.mark.parametrize("shape", [hr.SHAPES[3], hr.SHAPES[4]], ids=shape_id)
def test_the_float32_restatement_is_one_rounding_from_exact(shape):
    case = hr.make_case(np.float32, *shape)
    value, unit = hr.exact_reference(case)
    e = hr.errors(hr.reference(case), value, unit)
    assert np.nanmax(e) <= hr.bound(case, hr.numpy_worst(case))


# ---- the conditions on the cases, in exact arithmetic -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CLASS_SHAPES, ids=shape_id)
def test_the_cases_hold_every_class_and_every_bracket_is_the_exact_one(shape):
    """Every class occurs in every case of the thirteen heights (or more) with two levels at least; and in the finite float64 case every
    exact G is at least MARGIN |G| from every exact c[k] of its point, so that numpy's — and any correct kernel's — bracket is the exact
    one.  Measured: the smallest margin of these cases is 2.4e-6, and no (column, target) pair disagrees."""
    finite = hr.make_case(np.float64, *shape, False)
    if finite.n_lev >= 2 and finite.n_tgt >= len(hr.HEIGHTS_M):
        kinds = hr.classes(finite)
        assert {c for c in hr.CLASSES if (kinds == c).any()} == set(hr.CLASSES), shape
    smallest, disagreements = hr.margins(finite)
    print(f"{finite.name}: smallest margin {smallest:.3g}, {disagreements} bracket disagreements")
    assert smallest >= hr.MARGIN and disagreements == 0
    # the case with the planted values has the same columns apart from them: a NaN sp, a NaN zs above the sea, NaN and inf in t, q and x
    case = hr.make_case(np.float64, *shape)
    want = hr.reference(case)
    if case.n_pts > 11 and case.n_tgt >= len(hr.HEIGHTS_M):
        assert np.isnan(want[4]).all() and np.isnan(want[1]).any() and not np.isnan(want[0]).any()
        assert np.isnan(want[8]).all() == (case.reference == hr.SEA)
        assert np.isinf(want[10]).any() or np.isnan(want[10]).any()  # -inf at the bottom of point 10: copied, or inf - inf inside a bracket


def test_the_bent_case_is_not_monotone_and_its_brackets_are_exact():
    case = hr.bent_case(np.float64)
    bent = 0
    for col in range(case.n_columns):
        c = np.array(hr.column(case, col)[0])
        bent += bool(np.isfinite(c).all() and (np.diff(c) > 0).any())
    assert bent >= 8
    smallest, disagreements = hr.margins(case)
    assert smallest >= hr.MARGIN and disagreements == 0


def test_c_is_the_unrounded_geopotential_of_the_geopotential_restatement():
    """Above the sea c[k] has the bits of ``geopotential_restatement.column``; above the ground those of the same column without zs."""
    for reference in (hr.GROUND, hr.SEA):
        case = hr.make_case(np.float64, 48, 17, hr.SUBSET, 13, 1, reference, False)
        geo = case.geo if reference == hr.SEA else gr.GeoCase("no-zs", case.T, case.geo.A, case.geo.B, case.geo.sp, None, case.geo.t, case.geo.q)
        for col in (0, 7, 31):
            mine, theirs = np.array(hr.column(case, col)[0]), np.array(gr.column(geo, col))
            assert mine.tobytes() == theirs.tobytes()


def test_a_target_on_a_full_level_returns_that_level():
    """A target that equals numpy's own c[a] has w == 0: x[a]'s bits."""
    case = hr.on_level_case()
    got = hr.reference(case)
    chosen = ((0, 0), (0, 16), (12, 8), (20, 0), (20, 16), (33, 5))
    for i, (col, k) in enumerate(chosen):
        assert case.targets[i] == hr.column(case, col)[0][k]
        for v in range(case.n_var):
            assert got[col, v, i].tobytes() == case.x[col, v, k].tobytes(), (col, k, v)


# ---- planted defects ---------------------------------------------------------------------------------------------------------------
def defect_cases() -> list:
    return [hr.make_case(np.float64, 63, 2, hr.SUBSET, 13, 3, hr.GROUND), hr.make_case(np.float64, 65, 3, hr.WHOLE, 13, 2, hr.SEA),
            hr.make_case(np.float64, 48, 17, hr.WHOLE, 13, 2, hr.GROUND), hr.make_case(np.float64, 1, 1, hr.WHOLE, 1, 1, hr.SEA), hr.on_level_case()]


def test_the_restatement_passes_its_own_comparison():
    hr.check(lambda case, outside: hr.restate(case, outside), defect_cases(), hr.numpy_worst)


@pytest.mark.parametrize("defect", hr.DEFECTS)
def test_the_comparison_catches_a_planted_defect(defect):
    """Each wrong reading of the statement, planted in a copy of the restatement, fails the comparison the GPU test makes."""
    caught = []
    for case in defect_cases():
        try:
            hr.check(lambda c, outside: hr.restate(c, outside, defect=defect), [case], hr.numpy_worst)
        except AssertionError:
            caught.append(case.name)
    assert caught, f"no comparison notices {defect}"
    subset, sea, ground = (c.name for c in defect_cases()[:3])
    if defect == "first-ignored":
        assert caught == [subset]  # a whole model has first == 0
    if defect == "count-le":
        assert caught == [hr.on_level_case().name]  # only a target ON a level tells `<` from `<=`
    if defect == "ground-with-zs":
        assert sea not in caught and ground in caught
    if defect == "sea-without-zs":
        assert sea in caught and ground not in caught


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_agree():
    import abi_checks

    header = os.path.join(ROOT, "include", "atx_heights.h")
    declared = abi_checks.header_declarations(header, "ATX_HEIGHTS_API")
    assert declared == ["atx_heights_version", "atx_heights_last_error", "atx_heights_interpolate"]
    assert list(native_heights.SIGNATURES) == declared
    assert not set(declared) & (set(native.SIGNATURES) | set(native_levels.SIGNATURES) | set(native_geopotential.SIGNATURES))  # a library of its own
    text = open(header).read()
    assert native_heights.load().atx_heights_version() == 420 and "#define ATX_HEIGHTS_VERSION 420" in text
    assert f"#define ATX_HEIGHTS_MAX_LEVELS {native_heights.MAX_LEVELS}" in text
    assert native_heights.MAX_LEVELS == native_geopotential.MAX_LEVELS == native_levels.MAX_LEVELS
    assert "ATX_HEIGHTS_ABOVE_GROUND = 0, ATX_HEIGHTS_ABOVE_SEA = 1" in text and "ATX_HEIGHTS_NEAREST = 0, ATX_HEIGHTS_MISSING = 1" in text
    assert native_heights.REFERENCES == dict(ground=0, sea=1) and native_heights.OUTSIDE == dict(nearest=0, missing=1)
    assert "geopotential heights z / g, NOT geometric heights" in text and "unpinned" in text
    assert len(native_heights.SIGNATURES["atx_heights_interpolate"][1]) == 23
    if abi_checks.nm_tool():
        assert abi_checks.defined_dynamic_symbols(native_heights.lib_path())[0] == sorted(declared)
    import __graft_entry__ as graft

    assert [lib.binding for lib in graft.LIBRARIES].count("native_heights") == 1


def test_no_heights_kernel_uses_scratch_memory():
    """Read from the code objects inside libatx_heights.so (tools/kernel_resources.py; no GPU).  The LDS of the column kernels is asked
    for at the launch, so the fixed size is zero."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernel_resources(native_heights.lib_path())
    assert len([r for r in rows if "heights_columns_kernel" in r["name"]]) == 16  # 2 widths x (vector, scalar) for t x for q x for src
    assert len([r for r in rows if "heights_fields_kernel" in r["name"]]) == 2
    assert len(rows) == 18 and [r["name"] for r in rows if r["scratch"] > 0 or r["lds"] > 0] == []
    record = json.load(open(os.path.join(ROOT, "profiles", "heights_resources.json")))
    assert record["library"].endswith("libatx_heights.so") and len(record["kernels"]) == 18 and all(k["scratch"] == 0 for k in record["kernels"])


def test_abi_argument_validation_without_a_gpu():
    """Every refusal of include/atx_heights.h comes before anything touches HIP: the device pointers are never dereferenced."""
    lib = native_heights.load()
    fn = lib.atx_heights_interpolate
    at = lambda address: ctypes.c_void_p(address)  # noqa: E731 - never dereferenced: validation fails first, or there is nothing to do

    def call(src=at(4 << 20), out=at(3 << 20), t=at(1 << 20), q=at(2 << 20), sp=at(16), zs=at(32), A=at(48), B=at(64), targets=at(80), n_pts=8, n_var=2,
             n_lev=4, n_tgt=3, n_half=5, src_pitch=8, t_pitch=4, q_pitch=4, out_pitch=8, dtype=0, layout=0, reference=1, outside=0):
        return fn(src, out, t, q, sp, zs, A, B, targets, n_pts, n_var, n_lev, n_tgt, n_half, src_pitch, t_pitch, q_pitch, out_pitch, dtype, layout,
                  reference, outside, None)

    def said() -> str:
        return lib.atx_heights_last_error().decode()

    name = "atx_heights_interpolate"
    # unknown codes
    assert call(dtype=7) == native.EINVAL and said() == f"{name}: bad dtype 7"
    assert call(layout=5) == native.EINVAL and said() == f"{name}: bad layout 5"
    assert call(reference=2) == native.EINVAL and said() == f"{name}: unknown reference 2"
    assert call(outside=-1) == native.EINVAL and said() == f"{name}: unknown outside policy -1"
    # sizes
    for bad in (dict(n_pts=-1), dict(n_var=0), dict(n_lev=0), dict(n_tgt=-1)):
        assert call(**bad) == native.EINVAL and "bad sizes" in said()
    for bad in (1, 0, -3):
        assert call(n_half=bad) == native.EINVAL and said() == f"{name}: n_half={bad}: a model has at least one level, two half levels"
    assert call(n_half=4) == native.EINVAL and said() == f"{name}: n_lev=4 rows are the lowest levels of a model of 3, n_half=4"
    # null pointers of a call that is not empty
    for arg in ("src", "t", "q", "sp"):
        assert call(**{arg: None}) == native.EINVAL and said() == f"{name}: null src / t / q / sp pointer"
    assert call(out=None) == native.EINVAL and said() == f"{name}: null out pointer"
    assert call(targets=None) == native.EINVAL and said() == f"{name}: null targets"
    for arg in ("A", "B"):
        assert call(**{arg: None}) == native.EINVAL and said() == f"{name}: null A / B coefficients"
    assert call(zs=None) == native.EINVAL and said() == f"{name}: null zs above the sea"
    # (above the ground zs may be NULL: the call gets as far as the overlap check)
    assert call(zs=None, reference=0, out=at(1 << 20)) == native.EINVAL and said() == f"{name}: out overlaps t"
    # pitches too small for the shape, per stack, in both layouts
    for arg, least in (("src_pitch", 8), ("t_pitch", 4), ("q_pitch", 4), ("out_pitch", 6)):
        assert call(**{arg: least - 1}) == native.ESHAPE and "column pitch" in said() and "< rows (8, 4, 4, 6)" in said()
        assert call(**{arg: least}) != native.ESHAPE
        assert call(layout=1, **{**dict(src_pitch=8, t_pitch=8, q_pitch=8, out_pitch=8), arg: 7}) == native.ESHAPE and "field pitch" in said() and "< points 8" in said()
    # out's extent overlapping src's, t's or q's: 8 points x pitch 8 x 4 bytes = 256 bytes less the last point's padding
    for arg, base in (("src", 4 << 20), ("t", 1 << 20), ("q", 2 << 20)):
        for offset in (0, 100, -200):
            assert call(out=at(base + offset)) == native.EINVAL and said() == f"{name}: out overlaps {arg}"
    assert call(out=at((4 << 20) + 64), n_pts=0) == native.OK  # nothing to overlap in an empty call
    # beyond a stated limit: not implemented, never a silently wrong result
    assert call(n_lev=257, n_half=258, src_pitch=514, t_pitch=257, q_pitch=257) == native.ENOTIMPL and "exceeds the 256 levels of one call" in said()
    assert call(n_pts=2**31) == native.ENOTIMPL and call(n_half=65536) == native.ENOTIMPL
    assert call(n_var=65536, src_pitch=1 << 20, out_pitch=1 << 20) == native.ENOTIMPL
    assert call(n_tgt=65536, out_pitch=1 << 20) == native.ENOTIMPL
    assert call(n_var=20000, n_tgt=4, src_pitch=1 << 20, out_pitch=1 << 20) == native.ENOTIMPL and "exceed the indexing" in said()  # n_var x n_lev
    assert call(n_tgt=60000, out_pitch=1 << 20) == native.ENOTIMPL and "exceed the indexing" in said()  # n_var x n_tgt
    # one point's brackets beyond the LDS of a workgroup (validated before the launch; the pointers are far apart)
    far = dict(src=at(1 << 40), out=at(2 << 40), t=at(3 << 40), q=at(4 << 40))
    assert call(n_var=1, n_tgt=30000, src_pitch=4, out_pitch=30000, **far) == native.ENOTIMPL and "bytes of LDS" in said()
    # no points or no targets: validated, nothing launched
    assert call(src=None, out=None, t=None, q=None, sp=None, zs=None, n_pts=0) == native.OK
    assert call(out=None, targets=None, n_tgt=0, out_pitch=0) == native.OK
    assert call(src=None, out=None, t=None, q=None, sp=None, zs=None, n_pts=0, layout=9) == native.EINVAL  # ... validated all the same
    assert call(src=None, out=None, t=None, q=None, sp=None, zs=None, n_pts=0, n_half=139) == native.OK  # the lowest four levels of a longer table
    # the Python binding
    import torch

    z4, z8, AB = torch.zeros(4, 4), torch.zeros(4, 8), torch.zeros(5, dtype=torch.float64)
    kwargs = dict(n_pts=4, n_var=2, n_lev=4, n_tgt=3, src_pitch=8, t_pitch=4, q_pitch=4, out_pitch=8, layout=native.COLUMNS)
    with pytest.raises(RuntimeError, match="HBM-resident"):
        native_heights.interpolate(z8, z8.clone(), z4, z4.clone(), torch.zeros(4), None, AB, AB, torch.zeros(3, dtype=torch.float64), **kwargs)
    with pytest.raises(AssertionError):
        native_heights.interpolate(z8, z8.clone(), z4.double(), z4.clone(), torch.zeros(4), None, AB, AB, torch.zeros(3, dtype=torch.float64), **kwargs)
    with pytest.raises(ValueError, match="unknown reference 'air'"):
        native_heights.reference_code("air")
    with pytest.raises(ValueError, match="unknown outside policy"):
        native_heights.outside_code("clamp")


def test_interpolate_to_heights_checks_its_stacks_on_the_host():
    import torch

    from anemoi_transform_amd.stack import Stack
    from anemoi_transform_amd.vertical import G, interpolate_to_heights

    assert G == 9.80665 == hr.G
    x = Stack(torch.zeros(4, 8), 4, 8, native.COLUMNS)
    t = Stack(torch.zeros(4, 4), 4, 4, native.COLUMNS)
    AB = np.zeros(5)
    with pytest.raises(ValueError, match="does not hold 3 variables"):
        interpolate_to_heights(x, t, t, torch.zeros(4), None, AB, AB, [10.0], n_var=3)
    with pytest.raises(ValueError, match="t and q differ in shape or layout"):
        interpolate_to_heights(x, t, Stack(torch.zeros(4, 4), 4, 3, native.COLUMNS), torch.zeros(4), None, AB, AB, [10.0], n_var=2)
    with pytest.raises(ValueError, match="do not hold the 8 levels"):
        interpolate_to_heights(x, t, t, torch.zeros(4), None, AB, AB, [10.0])
    with pytest.raises(ValueError, match="do not hold the 4 levels"):
        interpolate_to_heights(x, Stack(torch.zeros(4, 4), 4, 4, native.FIELDS), Stack(torch.zeros(4, 4), 4, 4, native.FIELDS), torch.zeros(4), None, AB, AB,
                               [10.0], n_var=2)
    with pytest.raises(ValueError, match="differ in type"):
        d = Stack(torch.zeros(4, 4, dtype=torch.float64), 4, 4, native.COLUMNS)
        interpolate_to_heights(x, d, d, torch.zeros(4), None, AB, AB, [10.0], n_var=2)
    with pytest.raises(ValueError, match="unknown reference"):
        interpolate_to_heights(x, t, t, torch.zeros(4), None, AB, AB, [10.0], n_var=2, reference="air")
    with pytest.raises(ValueError, match="unknown outside policy"):
        interpolate_to_heights(x, t, t, torch.zeros(4), None, AB, AB, [10.0], n_var=2, outside="clamp")
    with pytest.raises(ValueError, match="need the surface geopotential"):
        interpolate_to_heights(x, t, t, torch.zeros(4), None, AB, AB, [10.0], n_var=2, reference="sea")
    with pytest.raises(AssertionError, match="same shape"):
        interpolate_to_heights(x, t, t, torch.zeros(4), None, AB, np.zeros(6), [10.0], n_var=2)
    with pytest.raises(AssertionError, match="at least one more vertical level"):
        interpolate_to_heights(x, t, t, torch.zeros(4), None, np.zeros(4), np.zeros(4), [10.0], n_var=2)
    with pytest.raises(AssertionError, match="sp"):
        interpolate_to_heights(x, t, t, torch.zeros(5), None, AB, AB, [10.0], n_var=2)


# ---- the filter --------------------------------------------------------------------------------------------------------------------
AB = dict(A=[0.0, 2000.0, 4000.0, 0.0], B=[0.0, 0.1, 0.5, 1.0])  # three model levels
NAME = "ml_to_hl"


def test_the_filter_is_registered_and_checks_its_configuration():
    assert NAME in filter_registry.registered
    f = create_filter_by_name(NAME, model_level_AB=AB)
    assert f.levels == [10, 100, 200] and all(isinstance(v, int) for v in f.levels) and f.heights_m == [10.0, 100.0, 200.0]
    assert (f.reference, f.outside, f.temperature, f.specific_humidity, f.surface_pressure, f.surface_geopotential, f.params) == (
        "ground", "nearest", "t", "q", "sp", "z", None)
    assert create_filter_by_name(NAME, levels=[2, 10.5], model_level_AB=AB).levels == [2, 10.5]
    assert create_filter_by_name(NAME, levels=100, model_level_AB=AB, params="u").params == ["u"]
    assert create_filter_by_name(NAME, levels=[-20, 0, 1500], model_level_AB=AB, reference="sea").levels == [-20, 0, 1500]
    with pytest.raises(ValueError, match="ml_to_hl: levels must be heights in metres"):
        create_filter_by_name(NAME, levels=["low"], model_level_AB=AB)
    with pytest.raises(ValueError, match="ml_to_hl: levels must be a non-empty list of finite heights"):
        create_filter_by_name(NAME, levels=[], model_level_AB=AB)
    with pytest.raises(ValueError, match="non-empty list of finite heights"):
        create_filter_by_name(NAME, levels=[10, float("nan")], model_level_AB=AB)
    with pytest.raises(ValueError, match="must not be negative above the ground"):
        create_filter_by_name(NAME, levels=[-5, 10], model_level_AB=AB)
    with pytest.raises(ValueError, match="ml_to_hl: duplicate levels"):
        create_filter_by_name(NAME, levels=[10, 10.0], model_level_AB=AB)
    with pytest.raises(ValueError, match="reference must be one of 'ground', 'sea'"):
        create_filter_by_name(NAME, model_level_AB=AB, reference="air")
    with pytest.raises(ValueError, match="outside must be one of 'nearest', 'missing'"):
        create_filter_by_name(NAME, model_level_AB=AB, outside="clamp")
    with pytest.raises(ValueError, match="three params"):
        create_filter_by_name(NAME, model_level_AB=AB, temperature="q")
    with pytest.raises(ValueError, match="same length"):
        create_filter_by_name(NAME, model_level_AB=dict(A=[0.0, 1.0], B=[0.0, 0.5, 1.0]))
    with pytest.raises(KeyError, match="predefined AB-coefficients"):
        create_filter_by_name(NAME, model_level_AB="IFS_137")


T3 = [("t", "ml", 1), ("t", "ml", 2), ("t", "ml", 3)]
Q3 = [("q", "ml", 1), ("q", "ml", 2), ("q", "ml", 3)]
U3 = [("u", "ml", 1), ("u", "ml", 2), ("u", "ml", 3)]
SP = ("sp", "sfc", None)


def test_grouping_errors_come_before_any_launch():
    """Host fields, no GPU here: each of these raises from the bookkeeping, before a stack is built or a kernel launched."""
    f = create_filter_by_name(NAME, model_level_AB=AB)
    with pytest.raises(ValueError, match="no surface pressure 'sp'") as no_sp:
        f.forward(fields(*T3, *Q3))
    assert "lnsp" not in str(no_sp.value)
    with pytest.raises(ValueError, match=r"no surface pressure 'sp'.*lnsp_to_sp \| ml_to_hl"):
        f.forward(fields(*T3, *Q3, ("lnsp", "ml", 1)))
    with pytest.raises(ValueError, match="ml_to_hl: no model-level fields of 'q'"):
        f.forward(fields(*T3, SP))
    with pytest.raises(ValueError, match="no model-level fields of 't'"):
        f.forward(fields(*Q3, *U3, SP))
    with pytest.raises(ValueError, match=r"mixed level sets for t and q: \[1, 2, 3\] and \[2, 3\]"):
        f.forward(fields(*T3, *Q3[1:], SP))
    with pytest.raises(ValueError, match=r"mixed level sets for t and u: \[1, 2, 3\] and \[1, 3\].*params= selects"):
        f.forward(fields(*T3, *Q3, U3[0], U3[2], SP))
    with pytest.raises(ValueError, match=r"mixed level sets for t and z: \[1, 2, 3\] and \[1\]"):  # above the ground a z on ml is a variable like any other
        f.forward(fields(*T3, *Q3, SP, ("z", "ml", 1)))
    with pytest.raises(ValueError, match=r"gap down to the lowest level 3 of the A / B table: missing levels \[2\]"):
        f.forward(fields(T3[0], T3[2], Q3[0], Q3[2], SP))
    with pytest.raises(ValueError, match=r"missing levels \[3\]"):
        f.forward(fields(*T3[:2], *Q3[:2], SP))
    with pytest.raises(ValueError, match="Duplicate component t .* level 2"):
        f.forward(fields(*T3, ("t", "ml", 2), *Q3, SP))
    with pytest.raises(ValueError, match="Duplicate component u .* level 1"):
        f.forward(fields(*T3, *Q3, *U3, U3[0], SP))
    with pytest.raises(ValueError, match="Duplicate component sp"):
        f.forward(fields(*T3, *Q3, SP, SP))
    with pytest.raises(ValueError, match="level 4 of u is outside the 3 model levels"):
        f.forward(fields(*T3, *Q3, ("u", "ml", 4), SP))
    two_dates = list(fields(*T3, *Q3, SP)) + list(fields(*T3, *Q3, date=20260102))
    with pytest.raises(ValueError, match="no surface pressure 'sp'.*20260102"):
        f.forward(two_dates)
    # above the sea: the group's ONE field of the surface geopotential
    sea = create_filter_by_name(NAME, model_level_AB=AB, reference="sea")
    with pytest.raises(ValueError, match="ml_to_hl: no surface geopotential 'z'"):
        sea.forward(fields(*T3, *Q3, SP))
    with pytest.raises(ValueError, match=r"2 fields of the surface geopotential 'z'.*geopotential_on_model_levels.*another output="):
        sea.forward(fields(*T3, *Q3, SP, ("z", "ml", 1), ("z", "sfc", None)))
    with pytest.raises(ValueError, match=r"3 fields of the surface geopotential 'z'.*another output="):  # what geopotential_on_model_levels leaves by default
        sea.forward(fields(*T3, *Q3, SP, ("z", "ml", 1), ("z", "ml", 2), ("z", "ml", 3)))


def test_the_plan_of_a_good_list():
    """Every input passes through, in input order; the columns top first; t and q are variables like any other unless ``params`` says
    otherwise; sp and lnsp are never interpolated; the template of a param is its first ml field of the input."""
    f = create_filter_by_name(NAME, model_level_AB=AB)
    data = fields(("q", "ml", 2), ("t", "ml", 3), SP, ("t", "ml", 1), ("2t", "sfc", None), ("u", "ml", 3), ("q", "ml", 3), ("t", "ml", 2), ("q", "ml", 1),
                  ("u", "ml", 1), ("u", "ml", 2), ("lnsp", "ml", 1), ("u", "pl", 850))
    passed, plan = f._plan(list(data))
    assert all(a is b for a, b in zip(passed, data)) and len(passed) == len(data)
    (group,) = plan
    assert group["levels"] == [1, 2, 3] and list(group["ml"]) == ["q", "t", "u"] and group["zs"] is None
    for key in ("t", "q"):
        assert [g.metadata("levelist") for g in group[key]] == [1, 2, 3] and {g.metadata("param") for g in group[key]} == {key}
    assert [g.metadata("levelist") for g in group["ml"]["u"]] == [1, 2, 3]
    assert {p: g.metadata("levelist") for p, g in group["templates"].items()} == dict(q=2, t=3, u=3)
    only_u = create_filter_by_name(NAME, model_level_AB=AB, params=["u"])
    (group,) = only_u._plan(list(data))[1]
    assert list(group["ml"]) == ["u"] and len(group["t"]) == len(group["q"]) == 3
    # a subset that reaches the ground; above the sea the one z of any levtype is the surface field, and is not interpolated
    sea = create_filter_by_name(NAME, model_level_AB=AB, reference="sea")
    (group,) = sea._plan(list(fields(*T3[1:], *Q3[1:], SP, ("z", "ml", 1))))[1]
    assert group["levels"] == [2, 3] and group["zs"].metadata("param") == "z" and list(group["ml"]) == ["t", "q"]
    (group,) = sea._plan(list(fields(*T3, *Q3, SP, ("z", "sfc", None))))[1]
    assert group["zs"].metadata("levtype") == "sfc"
    # above the ground a z on ALL the model levels is a variable
    (group,) = f._plan(list(fields(*T3, *Q3, SP, ("z", "ml", 1), ("z", "ml", 2), ("z", "ml", 3))))[1]
    assert list(group["ml"]) == ["t", "q", "z"]
    assert f._plan(list(fields(("2t", "sfc", None), ("u", "pl", 500))))[1] == []  # no ml field: nothing to do, nothing to miss
    assert only_u._plan(list(fields(*T3, *Q3)))[1] == []  # nothing selected: not even a surface pressure is missed


def test_the_unpinned_note_is_said_once(caplog):
    from anemoi_transform_amd.core import reset_notes

    def notes(fresh):
        if fresh:
            reset_notes()
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger="anemoi_transform_amd"):
            create_filter_by_name(NAME, model_level_AB=AB)
        return [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING and "unpinned" in r.getMessage()]

    said = notes(True)
    assert len(said) == 1 and "in-tree" in said[0] and "include/atx_heights.h" in said[0] and "earthkit-meteo" in said[0] and "z / g" in said[0]
    assert notes(False) == []  # once per process
