"""Geopotential on model levels without a GPU: the restatement of include/atx_geopotential.h (tests/geopotential_restatement.py) against exact
arithmetic, a closed form and the older column restatement, once as it is and once per planted defect through the comparison the GPU test
uses; numpy's own worst error per class, pinned; then the C ABI's argument validation through ctypes, the kernels' resources, and the
errors of the ``geopotential_on_model_levels`` filter.
"""

from __future__ import annotations

import ctypes
import json
import logging
import os

import mpmath
import numpy as np
import pytest

from anemoi_transform_amd import native, native_geopotential, native_levels
from anemoi_transform_amd.core import filter_registry
from anemoi_transform_amd.filters import create_filter_by_name

import geopotential_restatement as gr
import vertical_restatement as vr
from hybrid_column_common import fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# numpy's float64 arithmetic (the restatement before its rounding) against the exact statement on the float64 case of the class, in ulps
# of U: what the kernel's bounds (tests/test_gpu_geopotential.py) are relative to.  Measured here on the CPU, never from the kernel.  The
# conditioning of alpha is the cause of the large ones (1 - x with x near 1 in thin layers), as in tests/test_gpu_column_ulps.py; level
# 0 alone has no logarithm and a few roundings.
NUMPY_WORST_GEOPOTENTIAL = {
    (1, gr.WHOLE): 2.09, (1, gr.SUBSET): 24.43,
    (2, gr.WHOLE): 2.44, (2, gr.SUBSET): 29.87,
    (3, gr.WHOLE): 2.92, (3, gr.SUBSET): 63.33,
    (60, gr.WHOLE): 850.05, (60, gr.SUBSET): 2474.12,
    (137, gr.WHOLE): 2147.75, (137, gr.SUBSET): 13173.64,
}


def class_case(n_lev: int, kind: str) -> gr.GeoCase:
    """The float64 case of the class among the shared shapes."""
    with_zs = {(n, k): z for n, k, _, z in gr.SHAPES}[(n_lev, kind)]
    return gr.make_case(np.float64, n_lev, kind, with_zs)


# ---- numpy's own error, pinned ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [gr.WHOLE, gr.SUBSET])
@pytest.mark.parametrize("n_lev", gr.N_LEVS)
def test_numpy_worst_error_is_pinned(n_lev, kind):
    case = class_case(n_lev, kind)
    value, _ = gr.exact_reference(case)
    want = gr.reference(case)
    finite = np.isfinite(want)
    assert np.array_equal(np.vectorize(lambda v: v is not None, otypes=[bool])(value), finite), "the exact statement is a number where numpy's is"
    assert finite.mean() > 0.8
    worst, pinned = gr.numpy_worst(case), NUMPY_WORST_GEOPOTENTIAL[(n_lev, kind)]
    print(f"geopotential n_lev {n_lev} {kind}: numpy {worst:.4f} ulps of U")
    assert 0.8 * pinned <= worst <= 1.1 * pinned + 0.1, (n_lev, kind, worst, pinned)


@pytest.mark.parametrize("n_lev,kind", [(3, gr.SUBSET), (60, gr.WHOLE)])
def test_the_float32_restatement_is_one_rounding_from_exact(n_lev, kind):
    case = gr.make_case(np.float32, n_lev, kind)
    value, unit = gr.exact_reference(case)
    e = gr.errors(gr.reference(case), value, unit)
    assert np.nanmax(e) <= gr.bound(case, NUMPY_WORST_GEOPOTENTIAL[(n_lev, kind)])


def test_the_cases_hold_what_they_are_for():
    case = gr.make_case(np.float64, 60, gr.WHOLE)
    z = gr.reference(case)
    assert (case.zs < 0).any() and case.zs.max() >= 1e6 and (z[np.isfinite(z)] < 0).any()  # zs negative and large; z cancels against it
    mid = case.n_lev // 2
    for column in (1, 5):  # a NaN planted mid-column: it and every level above are NaN, nothing below
        assert np.isnan(z[column, : mid + 1]).all() and np.isfinite(z[column, mid + 1:]).all()
    assert np.isposinf(z[2, 0]) and np.isfinite(z[2, 1:]).all()  # +inf in t at the top stays there
    assert np.isnan(z[3]).all() and np.isnan(z[4]).all()  # -inf in q at the ground (inf - inf); a NaN sp
    assert {n for n, *_ in gr.SHAPES} == set(gr.N_LEVS) and {k for _, k, *_ in gr.SHAPES} == {gr.WHOLE, gr.SUBSET}
    assert {n for _, _, n, _ in gr.SHAPES} == {1, 63, 65, 257, 513} and {z for *_, z in gr.SHAPES} == {True, False}
    assert gr.make_case(np.float64, 137, gr.SUBSET).first == gr.SUBSET_ABOVE and gr.make_case(np.float64, 137, gr.WHOLE).first == 0


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [gr.WHOLE, gr.SUBSET])
def test_the_isothermal_dry_column_has_a_closed_form(kind):
    """t = T, q = 0: the deltas below a level telescope to ln(sp / p_dn), so z[k] = zs + Rd T (ln(sp / p_dn[k]) + alpha[k])."""
    base = gr.make_case(np.float64, 60, kind, specials=False)
    T0 = 273.0
    case = gr.GeoCase(f"isothermal-{kind}", np.float64, base.A, base.B, base.sp, base.zs, np.full_like(base.t, T0), np.zeros_like(base.q))
    value, unit = gr.exact(case)
    got = gr.restate(case)
    mp = mpmath.mpf
    worst = 0.0
    with mpmath.workprec(240):
        for p in range(case.n_pts):
            s, zs = mp(float(case.sp[p])), mp(float(case.zs[p]))
            for k in range(case.n_lev):
                j = case.first + k
                p_up, p_dn = mp(float(case.A[j])) + mp(float(case.B[j])) * s, mp(float(case.A[j + 1])) + mp(float(case.B[j + 1])) * s
                alpha = mpmath.log(2) if j == 0 else 1 - p_up / (p_dn - p_up) * mpmath.log(p_dn / p_up)
                closed = zs + mp(gr.RD) * mp(T0) * (mpmath.log(s / p_dn) + alpha)
                assert abs(value[p, k] - closed) <= abs(closed) * mp(10) ** -60 + mp(10) ** -60, (p, k)
                worst = max(worst, float(abs(mp(float(got[p, k])) - closed) / unit[p, k]))
    # the closed form pins the EXACT evaluator (above); numpy's arithmetic on these other columns is only held to the magnitude of the
    # class's pinned error — a hundred times it would be a wrong reading, not rounding
    assert worst <= 100.0 * NUMPY_WORST_GEOPOTENTIAL[(60, kind)], worst


@pytest.mark.parametrize("n_lev", gr.N_LEVS)
def test_without_zs_the_bottom_row_is_the_lowest_term_of_the_column_restatement(n_lev):
    """z of the lowest level is alpha r t of that level: ``vertical_restatement.relative_geopotential_thickness(...)[n - 1]``, the one
    level on which the reading of atx_pressure_at_height_stack and this statement agree — bit for bit."""
    case = gr.make_case(np.float64, n_lev, gr.WHOLE, with_zs=False)
    _, _, alpha = vr.pressure_at_model_levels(case.A, case.B, case.sp)
    want = vr.relative_geopotential_thickness(alpha, case.t.T, case.q.T)[n_lev - 1]
    gr.assert_same_bits(gr.reference(case)[:, n_lev - 1], want, f"bottom row, {n_lev} levels")
    if n_lev > 1:  # ... and only there: one level up the older reading is about half the thickness short
        above = vr.relative_geopotential_thickness(alpha, case.t.T, case.q.T)[n_lev - 2]
        assert (gr.reference(case)[0, n_lev - 2] > 1.2 * above[0])


# ---- planted defects ---------------------------------------------------------------------------------------------------------------
def defect_cases() -> list:
    return [gr.make_case(np.float64, 3, gr.WHOLE), gr.make_case(np.float64, 3, gr.SUBSET), gr.make_case(np.float64, 60, gr.WHOLE),
            gr.make_case(np.float64, 1, gr.WHOLE)]


def test_the_restatement_passes_its_own_comparison():
    gr.check(lambda case: gr.restate(case), defect_cases(), NUMPY_WORST_GEOPOTENTIAL)


@pytest.mark.parametrize("defect", gr.DEFECTS)
def test_the_comparison_catches_a_planted_defect(defect):
    """Each wrong reading of the statement, planted in a copy of the restatement, fails the comparison the GPU test makes."""
    caught = []
    for case in defect_cases():
        try:
            gr.check(lambda c: gr.restate(c, defect=defect), [case], NUMPY_WORST_GEOPOTENTIAL)
        except AssertionError:
            caught.append(case.name)
    assert caught, f"no comparison notices {defect}"
    if defect == "first-ignored":
        assert caught == [gr.make_case(np.float64, 3, gr.SUBSET).name]  # a whole model has first == 0
    if defect == "top-general":
        assert gr.make_case(np.float64, 3, gr.SUBSET).name not in caught  # a subset has no level 0


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_agree():
    import abi_checks

    header = os.path.join(ROOT, "include", "atx_geopotential.h")
    declared = abi_checks.header_declarations(header, "ATX_GEOPOTENTIAL_API")
    assert declared == ["atx_geopotential_version", "atx_geopotential_last_error", "atx_geopotential_on_model_levels"]
    assert list(native_geopotential.SIGNATURES) == declared
    assert not set(declared) & (set(native.SIGNATURES) | set(native_levels.SIGNATURES))  # a library of its own: libatx_levels keeps its three
    assert native_geopotential.load().atx_geopotential_version() == 420 and "#define ATX_GEOPOTENTIAL_VERSION 420" in open(header).read()
    assert f"#define ATX_GEOPOTENTIAL_MAX_LEVELS {native_geopotential.MAX_LEVELS}" in open(header).read()
    assert native_geopotential.MAX_LEVELS == native_levels.MAX_LEVELS  # what ml_to_pl takes, this takes
    assert len(native_geopotential.SIGNATURES["atx_geopotential_on_model_levels"][1]) == 16
    if abi_checks.nm_tool():
        assert abi_checks.defined_dynamic_symbols(native_geopotential.lib_path())[0] == sorted(declared)
    import __graft_entry__ as graft

    assert [lib.binding for lib in graft.LIBRARIES].count("native_geopotential") == 1


def test_no_geopotential_kernel_uses_scratch_memory():
    """Read from the code objects inside libatx_geopotential.so (tools/kernel_resources.py; no GPU).  The LDS of the column kernels is asked
    for at the launch, so the fixed size is zero."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernel_resources(native_geopotential.lib_path())
    assert len([r for r in rows if "geopotential_columns_kernel" in r["name"]]) == 8  # 2 widths x (vector, scalar) for t x the same for q
    assert len([r for r in rows if "geopotential_fields_kernel" in r["name"]]) == 2
    assert len(rows) == 10 and [r["name"] for r in rows if r["scratch"] > 0 or r["lds"] > 0] == []
    record = json.load(open(os.path.join(ROOT, "profiles", "geopotential_resources.json")))
    assert record["library"].endswith("libatx_geopotential.so") and len(record["kernels"]) == 10 and all(k["scratch"] == 0 for k in record["kernels"])


def test_abi_argument_validation_without_a_gpu():
    """Every refusal of include/atx_geopotential.h comes before anything touches HIP: the device pointers are never dereferenced."""
    lib = native_geopotential.load()
    fn = lib.atx_geopotential_on_model_levels
    at = lambda address: ctypes.c_void_p(address)  # noqa: E731 - never dereferenced: validation fails first, or there are no points

    def call(t=at(1 << 20), q=at(2 << 20), sp=at(16), zs=at(32), A=at(48), B=at(64), out=at(3 << 20), n_pts=8, n_lev=4, n_half=5, t_pitch=4,
             q_pitch=4, out_pitch=4, dtype=0, layout=0):
        return fn(t, q, sp, zs, A, B, out, n_pts, n_lev, n_half, t_pitch, q_pitch, out_pitch, dtype, layout, None)

    def said() -> str:
        return lib.atx_geopotential_last_error().decode()

    name = "atx_geopotential_on_model_levels"
    # null pointers of a call that is not empty (zs may be NULL: 0.0 everywhere — it gets as far as the overlap check below)
    for arg in ("t", "q", "sp"):
        assert call(**{arg: None}) == native.EINVAL and said() == f"{name}: null t / q / sp pointer"
    assert call(out=None) == native.EINVAL and said() == f"{name}: null out pointer"
    for arg in ("A", "B"):
        assert call(**{arg: None}) == native.EINVAL and said() == f"{name}: null A / B coefficients"
    # sizes
    assert call(n_lev=0) == native.EINVAL and "bad sizes" in said()
    assert call(n_pts=-1) == native.EINVAL and "bad sizes" in said()
    for bad in (1, 0, -3):
        assert call(n_half=bad) == native.EINVAL and said() == f"{name}: n_half={bad}: a model has at least one level, two half levels"
    assert call(n_half=4) == native.EINVAL and said() == f"{name}: n_lev=4 rows are the lowest levels of a model of 3, n_half=4"
    # unknown codes
    assert call(dtype=7) == native.EINVAL and said() == f"{name}: bad dtype 7"
    assert call(layout=5) == native.EINVAL and said() == f"{name}: bad layout 5"
    # pitches too small for the shape, per stack, in both layouts
    for arg in ("t_pitch", "q_pitch", "out_pitch"):
        assert call(**{arg: 3}) == native.ESHAPE and "column pitch" in said() and "< rows 4" in said()
        assert call(layout=1, **{**dict(t_pitch=8, q_pitch=8, out_pitch=8), arg: 7}) == native.ESHAPE and "field pitch" in said() and "< points 8" in said()
    # out's extent overlapping t's or q's: 8 points x pitch 4 x 4 bytes = 128 bytes (the last point's padding is outside the extent)
    base = 1 << 20
    assert call(out=at(base)) == native.EINVAL and said() == f"{name}: out overlaps t"
    assert call(out=at(base + 124)) == native.EINVAL and said() == f"{name}: out overlaps t"
    assert call(out=at(base - 124)) == native.EINVAL and said() == f"{name}: out overlaps t"
    assert call(out=at((2 << 20) + 64), zs=None) == native.EINVAL and said() == f"{name}: out overlaps q"
    assert call(out=at(base + 64), dtype=1, n_pts=0) == native.OK  # nothing to overlap in an empty call
    # beyond a stated limit: not implemented, never a silently wrong result
    assert call(n_lev=257, n_half=258, t_pitch=257, q_pitch=257, out_pitch=257) == native.ENOTIMPL and "exceeds the 256 levels of one call" in said()
    assert call(n_pts=2**31, layout=0) == native.ENOTIMPL and call(n_half=65536) == native.ENOTIMPL
    # no points: validated, nothing launched
    assert call(t=None, q=None, sp=None, zs=None, out=None, n_pts=0) == native.OK
    assert call(t=None, q=None, sp=None, out=None, n_pts=0, layout=9) == native.EINVAL  # ... validated all the same
    assert call(t=None, q=None, sp=None, out=None, n_pts=0, n_lev=4, n_half=139) == native.OK  # the lowest four levels of a longer table
    # the Python binding
    import torch

    z4, AB = torch.zeros(4, 4), torch.zeros(5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="HBM-resident"):
        native_geopotential.geopotential(z4, z4.clone(), torch.zeros(4), None, AB, AB, z4.clone(), n_pts=4, n_lev=4, t_pitch=4, q_pitch=4, out_pitch=4,
                                   layout=native.COLUMNS)
    with pytest.raises(AssertionError):
        native_geopotential.geopotential(z4, z4.double(), torch.zeros(4), None, AB, AB, z4.clone(), n_pts=4, n_lev=4, t_pitch=4, q_pitch=4, out_pitch=4,
                                   layout=native.COLUMNS)


def test_geopotential_on_model_levels_checks_its_stacks_on_the_host():
    import torch

    from anemoi_transform_amd.stack import Stack
    from anemoi_transform_amd.vertical import geopotential_on_model_levels

    t = Stack(torch.zeros(4, 4), 4, 4, native.COLUMNS)
    with pytest.raises(ValueError, match="differ in shape or layout"):
        geopotential_on_model_levels(t, Stack(torch.zeros(4, 4), 4, 3, native.COLUMNS), torch.zeros(4), None, np.zeros(5), np.zeros(5))
    with pytest.raises(ValueError, match="differ in shape or layout"):
        geopotential_on_model_levels(t, Stack(torch.zeros(4, 4), 4, 4, native.FIELDS), torch.zeros(4), None, np.zeros(5), np.zeros(5))
    with pytest.raises(ValueError, match="differ in type"):
        geopotential_on_model_levels(t, Stack(torch.zeros(4, 4, dtype=torch.float64), 4, 4, native.COLUMNS), torch.zeros(4), None, np.zeros(5), np.zeros(5))
    with pytest.raises(AssertionError, match="same shape"):
        geopotential_on_model_levels(t, t, torch.zeros(4), None, np.zeros(5), np.zeros(6))
    with pytest.raises(AssertionError, match="at least one more vertical level"):
        geopotential_on_model_levels(t, t, torch.zeros(4), None, np.zeros(4), np.zeros(4))
    with pytest.raises(AssertionError, match="sp"):
        geopotential_on_model_levels(t, t, torch.zeros(5), None, np.zeros(5), np.zeros(5))


# ---- the filter --------------------------------------------------------------------------------------------------------------------
AB = dict(A=[0.0, 2000.0, 4000.0, 0.0], B=[0.0, 0.1, 0.5, 1.0])  # three model levels
NAME = "geopotential_on_model_levels"


def test_the_filter_is_registered_and_checks_its_configuration():
    assert NAME in filter_registry.registered
    f = create_filter_by_name(NAME, model_level_AB=AB)
    assert (f.temperature, f.specific_humidity, f.surface_pressure, f.surface_geopotential, f.output) == ("t", "q", "sp", "z", "z")
    assert f.A.tolist() == AB["A"] and f.B.tolist() == AB["B"]
    with pytest.raises(ValueError, match="same length"):
        create_filter_by_name(NAME, model_level_AB=dict(A=[0.0, 1.0], B=[0.0, 0.5, 1.0]))
    with pytest.raises(ValueError, match="three params"):
        create_filter_by_name(NAME, model_level_AB=AB, temperature="q")
    with pytest.raises(KeyError, match="predefined AB-coefficients"):
        create_filter_by_name(NAME, model_level_AB="IFS_137")
    with pytest.raises(TypeError, match="string or a dictionary"):
        create_filter_by_name(NAME, model_level_AB=[1, 2])
    from anemoi_transform_amd.filters import vertical

    assert vertical.GEOPOTENTIAL_COLUMNS_ROUTE in ("columns", "fields")


T3 = [("t", "ml", 1), ("t", "ml", 2), ("t", "ml", 3)]
Q3 = [("q", "ml", 1), ("q", "ml", 2), ("q", "ml", 3)]
SFC = [("sp", "sfc", None), ("z", "ml", 1)]


def test_grouping_errors_come_before_any_launch():
    """Host fields, no GPU here: each of these raises from the bookkeeping, before a stack is built or a kernel launched."""
    f = create_filter_by_name(NAME, model_level_AB=AB)
    with pytest.raises(ValueError, match="no surface pressure 'sp'") as no_sp:
        f.forward(fields(*T3, *Q3, ("z", "ml", 1)))
    assert "lnsp" not in str(no_sp.value)
    with pytest.raises(ValueError, match=r"no surface pressure 'sp'.*lnsp_to_sp \| geopotential_on_model_levels"):
        f.forward(fields(*T3, *Q3, ("z", "ml", 1), ("lnsp", "ml", 1)))
    with pytest.raises(ValueError, match="no surface geopotential 'z'"):
        f.forward(fields(*T3, *Q3, ("sp", "sfc", None)))
    with pytest.raises(ValueError, match="no model-level fields of 'q'"):
        f.forward(fields(*T3, *SFC))
    with pytest.raises(ValueError, match="no model-level fields of 't'"):
        f.forward(fields(*Q3, *SFC))
    with pytest.raises(ValueError, match=r"mixed level sets for t and q: \[1, 2, 3\] and \[2, 3\]"):
        f.forward(fields(*T3, *Q3[1:], *SFC))
    with pytest.raises(ValueError, match=r"gap down to the lowest level 3 of the A / B table: missing levels \[2\]"):
        f.forward(fields(T3[0], T3[2], Q3[0], Q3[2], *SFC))
    with pytest.raises(ValueError, match=r"missing levels \[3\]"):
        f.forward(fields(*T3[:2], *Q3[:2], *SFC))
    with pytest.raises(ValueError, match="Duplicate component t .* level 2"):
        f.forward(fields(*T3, ("t", "ml", 2), *Q3, *SFC))
    with pytest.raises(ValueError, match="Duplicate component sp"):
        f.forward(fields(*T3, *Q3, *SFC, ("sp", "sfc", None)))
    with pytest.raises(ValueError, match="Duplicate component z"):
        f.forward(fields(*T3, *Q3, *SFC, ("z", "sfc", None)))
    with pytest.raises(ValueError, match="level 4 of t is outside the 3 model levels"):
        f.forward(fields(("t", "ml", 4), *Q3, *SFC))
    with pytest.raises(ValueError, match="level 0 of q is outside"):
        f.forward(fields(*T3, ("q", "ml", 0), *SFC))
    two_dates = list(fields(*T3, *Q3, *SFC)) + list(fields(*T3, *Q3, ("z", "ml", 1), date=20260102))
    with pytest.raises(ValueError, match="no surface pressure 'sp'.*20260102"):
        f.forward(two_dates)


def test_the_plan_of_a_good_list():
    """What passes through, in input order — everything but the surface z, whose (param, levtype, levelist) an output field takes — and
    the columns, top first; a subset keeps its surface z, and a surface z of another levtype passes whatever the levels."""
    f = create_filter_by_name(NAME, model_level_AB=AB)
    data = fields(("q", "ml", 2), ("t", "ml", 3), ("sp", "sfc", None), ("t", "ml", 1), ("2t", "sfc", None), ("z", "ml", 1), ("q", "ml", 3), ("t", "ml", 2),
                  ("q", "ml", 1), ("u", "ml", 1))
    passed, plan = f._plan(list(data))
    assert [(g.metadata("param"), g.metadata("levelist", default=None)) for g in passed] == [
        ("q", 2), ("t", 3), ("sp", None), ("t", 1), ("2t", None), ("q", 3), ("t", 2), ("q", 1), ("u", 1)]
    (group,) = plan
    assert group["levels"] == [1, 2, 3] and [g.metadata("levelist") for g in group["t"]] == [1, 2, 3] == [g.metadata("levelist") for g in group["q"]]
    assert group["sp"].metadata("param") == "sp" and group["zs"].metadata("param") == "z"
    subset = fields(*T3[1:], *Q3[1:], *SFC)
    passed, plan = f._plan(list(subset))
    assert len(passed) == len(subset) and plan[0]["levels"] == [2, 3]
    sfc_z = fields(*T3, *Q3, ("sp", "sfc", None), ("z", "sfc", None))
    passed, plan = f._plan(list(sfc_z))
    assert len(passed) == len(sfc_z) and plan[0]["zs"].metadata("levtype") == "sfc"
    renamed = create_filter_by_name(NAME, model_level_AB=AB, output="gh_ml")
    passed, _ = renamed._plan(list(data))
    assert len(passed) == len(data)
    assert f._plan(list(fields(("2t", "sfc", None), ("u", "ml", 1)))) [1] == []  # no t, no q: nothing to do, nothing to miss


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
    assert len(said) == 1 and "in-tree" in said[0] and "include/atx_geopotential.h" in said[0] and "earthkit-meteo" in said[0] and "MARS" in said[0]
    assert notes(False) == []  # once per process
