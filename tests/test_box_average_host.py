"""Grid-box-average regridding without a GPU: ``interp.box_average_rows(device=False)`` against the plain-loop restatement
(tests/box_average_restatement.py) with each of the restatement's defects caught by the check named for it, the ``regrid`` filter's
new methods, the ``atx make-regrid-file box-average-matrix`` command, and the header, binding, exports and argument checks of the
companion library ``libatx_plan``.
"""

from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import abi_checks
import box_average_restatement as R
from anemoi_transform_amd import cli, interp, native_plan
from anemoi_transform_amd.filters import create_filter_by_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "atx_plan.h")


def host(src_rows, tgt_rows):
    return interp.box_average_rows(src_rows, tgt_rows, device=False)


# ---- the statement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.PAIRS) + list(R.IDENTITIES))
def test_host_equals_the_restatement_and_holds_the_invariants(name):
    R.run_checks(host, pairs=[name])


def test_the_restatement_passes_its_own_checks():
    R.run_checks(R.box_average)


def test_the_sliver_pair_has_every_source_cell_once():
    m = host(R.rows_of([7.2, 7.2]), R.rows_of([36.0, 36.0]))
    assert len(m["matrix_indices"]) == 1300 == int(m["matrix_shape"][1])
    assert np.array_equal(np.sort(m["matrix_indices"]), np.arange(1300))


@pytest.mark.parametrize("name", sorted(R.IDENTITIES))
def test_identical_grids_give_the_identity(name):
    src, tgt = R.IDENTITIES[name]
    m = host(R.rows_of(src), R.rows_of(tgt))
    assert np.array_equal(m["matrix_indices"], np.arange(len(m["matrix_indices"]))) and np.all(m["matrix_data"] == 1.0)


def test_upsampling_rows_hold_one_to_four_entries():
    lengths = np.diff(host(R.rows_of([30.0, 30.0]), R.rows_of("O8"))["matrix_indptr"])
    assert lengths.min() == 1 and lengths.max() == 4


@pytest.mark.parametrize("defect", sorted(R.DEFECTS))
def test_the_checks_catch_every_defect(defect):
    with pytest.raises(AssertionError, match=R.DEFECTS[defect]):
        R.run_checks(lambda s, t: R.box_average(s, t, defect=defect))


def test_output_format_is_the_mir_triplet():
    m = host(R.rows_of("O8"), R.rows_of("F4"))
    assert sorted(m) == ["matrix_data", "matrix_indices", "matrix_indptr", "matrix_shape"]
    assert (m["matrix_data"].dtype, m["matrix_indices"].dtype, m["matrix_indptr"].dtype) == (np.float64, np.int32, np.int32)
    assert list(m["matrix_shape"]) == [128, 544]


@pytest.mark.parametrize("rows, message", [
    ((np.array([60.0, 0.0, -60.0]), np.array([4, 1, 4])), "at least 2 points"),
    ((np.array([60.0, 60.0, -60.0]), np.array([4, 4, 4])), "strictly decreasing"),
    ((np.array([-60.0, 0.0, 60.0]), np.array([4, 4, 4])), "strictly decreasing"),
    ((np.array([60.0, 0.0]), np.array([4, 4, 4])), "row structure"),
    ((np.array([60.0, 0.0]), np.array([4.0, 4.0])), "row structure"),
])
def test_malformed_rows_raise_value_error(rows, message):
    good = R.rows_of("O8")
    for args in ((rows, good), (good, rows)):
        with pytest.raises(ValueError, match=message):
            interp.box_average_rows(*args)


def test_device_true_without_a_gpu_raises():
    import torch

    if not torch.cuda.is_available():  # with a GPU, tests/test_gpu_box_average.py runs this call
        with pytest.raises(RuntimeError, match="device=False"):
            interp.box_average_rows(R.rows_of("O8"), R.rows_of("F4"), device=True)


# ---- the filter --------------------------------------------------------------------------------------------------------------------------
def test_filter_constructs_on_a_cpu_box(caplog):
    with caplog.at_level("WARNING"):
        f = create_filter_by_name("regrid", in_grid="O16", out_grid="O4", method="grid-box-average")
    plan = f.interpolator.plan
    assert type(f.interpolator).__name__ == "EarthkitRegrid" and (plan.n_src, plan.n_tgt) == (1600, 208)
    said = [r.getMessage() for r in caplog.records if "grid-box-average" in r.getMessage()]
    assert len(said) == 1 and "unpinned" in said[0]


def test_filter_needs_rows_on_both_sides(tmp_path):
    from anemoi_transform_amd.grids import lookup

    points = str(tmp_path / "points.npz")
    g = lookup("O4")
    np.savez(points, latitudes=g["latitudes"], longitudes=g["longitudes"])
    with pytest.raises(NotImplementedError, match="matrix") as caught:
        create_filter_by_name("regrid", in_grid="O16", out_grid=points, method="grid-box-average")
    assert "row-structured" in str(caught.value)
    with pytest.raises(NotImplementedError, match="matrix"):
        create_filter_by_name("regrid", in_grid=points, out_grid="O4", method="grid-box-average")
    with pytest.raises(NotImplementedError, match="matrix"):
        create_filter_by_name("regrid", in_grid="o32", out_grid="o48", method="conservative")


def test_nearest_neighbour_is_the_k1_search(caplog):
    from anemoi_transform_amd.grids import lookup
    from anemoi_transform_amd.interp import nearest_grid_points

    with caplog.at_level("WARNING"):
        f = create_filter_by_name("regrid", in_grid="O8", out_grid=[30.0, 30.0], method="nearest-neighbour")
    plan = f.interpolator.plan
    src, tgt = lookup("O8"), lookup([30.0, 30.0])
    want = nearest_grid_points(src["latitudes"], src["longitudes"], tgt["latitudes"], tgt["longitudes"])
    assert plan.kind == "ell" and plan.k == 1 and np.array_equal(plan.index.reshape(-1), want.reshape(-1))
    assert sum("unpinned" in r.getMessage() for r in caplog.records) == 1


# ---- the command -------------------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_matrix_file(tmp_path):
    path = str(tmp_path / "m.npz")
    assert cli.main(["make-regrid-file", "box-average-matrix", "O16", "O4", "--output", path]) == 0
    loaded = interp.load_matrix_npz(path)
    assert sorted(loaded) == ["in_latitudes", "in_longitudes", "matrix_data", "matrix_indices", "matrix_indptr", "matrix_shape",
                              "out_latitudes", "out_longitudes"]
    R.check_equal(loaded, R.statement("O16->O4"), "O16->O4 from the file")
    assert loaded["in_latitudes"].shape == (1600,) and loaded["out_longitudes"].shape == (208,)
    plan = create_filter_by_name("regrid", matrix=path).interpolator.plan  # the file is what regrid(matrix=...) reads
    assert (plan.n_src, plan.n_tgt) == (1600, 208)
    with pytest.raises(SystemExit, match="row-structured"):
        cli.main(["make-regrid-file", "box-average-matrix", "O16", path, "--output", str(tmp_path / "n.npz")])


# ---- the C ABI of the companion library -------------------------------------------------------------------------------------------------
def header_declarations() -> list[str]:
    return abi_checks.header_declarations(HEADER, "ATX_PLAN_API")


def test_header_declares_the_binding():
    text = open(HEADER).read()
    assert header_declarations() == ["atx_plan_version", "atx_plan_last_error", "atx_plan_box_average_count", "atx_plan_box_average_fill"]
    assert sorted(native_plan.SIGNATURES) == sorted(header_declarations())
    assert re.search(r"#define ATX_PLAN_VERSION 420\b", text) and '#include "atx.h"' in text
    for name, n_args in (("atx_plan_box_average_count", 12), ("atx_plan_box_average_fill", 15)):
        declared = re.search(name + r"\(([^)]*)\);", text).group(1)
        assert len(declared.split(",")) == n_args == len(native_plan.SIGNATURES[name][1]), name


def test_header_is_plain_c99(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "use_header.c"
    src.write_text('#include "atx_plan.h"\nint use(void) { return ATX_PLAN_VERSION + ATX_OK + ATX_EINVAL; }\n')
    run = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "use_header.o")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


def malformed_calls(lib):
    """(entry point, arguments, word of the message) for every argument check of the two entry points: nothing is launched."""
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    tables = [one, one, one, 4, 40, one, one, one, 3, 12]  # zs, src_len, src_start, rows, n_src, zt, tgt_len, tgt_start, rows, n_tgt
    tails = {"count": [one, None], "fill": [one, 30, one, one, None]}
    for kind, tail in tails.items():
        call = getattr(lib, f"atx_plan_box_average_{kind}")
        for pos, bad, word in ((3, 0, b"rows"), (3, 2**31, b"rows"), (8, 0, b"rows"), (8, -1, b"rows"), (4, 0, b"n_src"),
                               (4, 2**31, b"n_src"), (9, -1, b"negative")):
            yield call, tables[:pos] + [bad] + tables[pos + 1:] + tail, word
        for pos in (0, 1, 2, 5, 6, 7):
            yield call, tables[:pos] + [None] + tables[pos + 1:] + tail, b"null"
    yield lib.atx_plan_box_average_count, tables + [None, None], b"null"
    fill = lib.atx_plan_box_average_fill
    for nnz in (-1, 2**31):
        yield fill, tables + [one, nnz, one, one, None], b"nnz"
    for tail in ([None, 30, one, one, None], [one, 30, None, one, None], [one, 30, one, None, None]):
        yield fill, tables + tail, b"null"


def test_abi_argument_validation_without_a_gpu():
    lib = native_plan.load()
    assert lib.atx_plan_version() == 420
    n = 0
    for call, args, word in malformed_calls(lib):
        assert call(*args) == native_plan.EINVAL and word in lib.atx_plan_last_error(), (args, lib.atx_plan_last_error())
        n += 1
    assert n == 2 * 13 + 1 + 2 + 3
    # no targets: nothing launched, no storage needed ... but the rest is still validated
    assert lib.atx_plan_box_average_count(None, None, None, 4, 40, None, None, None, 3, 0, None, None) == native_plan.OK
    assert lib.atx_plan_box_average_fill(None, None, None, 4, 40, None, None, None, 3, 0, None, 0, None, None, None) == native_plan.OK
    assert lib.atx_plan_box_average_count(None, None, None, 0, 40, None, None, None, 3, 0, None, None) == native_plan.EINVAL
    assert lib.atx_plan_box_average_fill(None, None, None, 4, 40, None, None, None, 3, 0, None, -1, None, None, None) == native_plan.EINVAL
