"""Linear regridding from unstructured source grids without a GPU: the walk (``interp.locate_walk_host``) against the independent
statement (``interp.locate_brute_host``) on the point sets of tests/linear_unstructured_cases.py, the properties of the matrix
``interp.linear_triangulated`` builds, the mesh ``interp.triangulate_sphere`` returns, targets outside the domain, the ``regrid``
filter's ``method="linear-unstructured"``, the ``atx make-regrid-file linear-matrix`` command, and the header, binding, exports and
argument checks of the companion library ``libatx_mesh``.
"""

from __future__ import annotations

import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.sparse import csr_array

import abi_checks
import linear_unstructured_cases as C
import native_double
from anemoi_transform_amd import cli, interp, native_mesh
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.grids import lookup
from oracle import oracle
from test_filters import synthetic_fields, test_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "atx_mesh.h")
ULP = np.finfo(np.float64).eps


def strictly_inside(c, tri_out, status, margin=1e-9):
    """Rows that the brute-force statement found with ``min_i d_i / D > margin``."""
    rows = np.flatnonzero(status == interp.FOUND)
    a, b, cc = (c.src_xyz[c.mesh["tri"][tri_out[rows], i]] for i in range(3))
    p = c.tgt_xyz[rows]
    least = np.minimum(np.minimum(interp._det(p, b, cc), interp._det(p, cc, a)), interp._det(p, a, b)) / interp._det(a, b, cc)
    return rows[least > margin]


# ---- the walk against brute force ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_walk_agrees_with_brute_force(name):
    c = C.case(name)
    tri_out, w, status, steps = c.walked
    brute_tri, _, brute_status = c.brute
    undecided = status == interp.UNDECIDED
    print(f"{name}: {len(status)} targets, status counts {np.bincount(status, minlength=4)}, at most {steps.max()} moves, "
          f"{int(c.mesh['flag'].sum())} of {len(c.mesh['tri'])} triangles flagged")
    assert set(np.unique(status)) <= {interp.FOUND, interp.UNDECIDED, interp.OUTSIDE}
    assert np.array_equal((status == interp.FOUND)[~undecided], (brute_status == interp.FOUND)[~undecided])
    strict = strictly_inside(c, brute_tri, brute_status)
    assert np.array_equal(tri_out[strict], brute_tri[strict]) and not undecided[strict].any()
    if name in C.GLOBAL:
        assert not undecided.any() and (status == interp.FOUND).all()
        assert steps.max() <= {"random": 6, "O32->5deg": 10}.get(name, 64)
    if name == "box":
        assert undecided.sum() <= 0.02 * len(status) and (brute_status[undecided] == interp.OUTSIDE).all()
        inside = (np.abs(c.tgt["latitudes"] - 50.0) <= 10.0) & (np.abs(c.tgt["longitudes"] - 5.0) <= 15.0)
        assert inside.sum() == 2501 and np.array_equal(status == interp.FOUND, inside)
    found = np.flatnonzero(status == interp.FOUND)
    assert C.direction_error(c, tri_out, w, found) <= 1e-12


@pytest.mark.parametrize("name", C.GLOBAL)
def test_a_grid_onto_itself_needs_no_move(name):
    tri_out, w, status, steps = C.self_case(name).walk()
    assert (status == interp.FOUND).all() and steps.max() == 0


def test_o96_to_one_degree_leaves_nothing_undecided():
    src, tgt = lookup("o96"), lookup([1.0, 1.0])
    src_xyz, tgt_xyz = (interp.unit_sphere_xyz(g["latitudes"], g["longitudes"]) for g in (src, tgt))
    mesh = interp.triangulate_sphere(src_xyz)
    hull = mesh["hull_vertices"]
    seed = mesh["vertex_tri"][hull[interp._nearest_by_index(src_xyz[hull], tgt_xyz)]]
    _, _, status, _ = interp.locate_walk_host(src_xyz, mesh["tri"], mesh["nbr"], mesh["flag"], tgt_xyz, seed)
    assert (status == interp.FOUND).all()


def test_max_steps_bounds_the_walk_and_the_fallback_restores_the_matrix():
    c = C.case("O32->5deg")
    full = c.walked
    for max_steps in (0, 2):
        tri_out, w, status, steps = c.walk(max_steps)
        done = full[3] <= max_steps
        assert np.array_equal(status == interp.FOUND, done) and (status[~done] == interp.UNDECIDED).all() and (~done).any()
        assert steps.max() == max_steps and np.array_equal(tri_out[done], full[0][done]) and np.array_equal(w[done], full[1][done])
        assert not w[~done].any()
        bounded = interp.linear_triangulated(c.src, c.tgt, max_steps=max_steps)  # the undecided rows resume the walk on the host
        assert all(np.array_equal(bounded[k], matrix_of("O32->5deg")[k]) for k in bounded)


def test_a_malformed_seed_or_neighbour_ends_that_row_alone():
    c = C.case("random")
    want = c.walked
    moved = int(np.flatnonzero(want[3] > 0)[0])
    seed, nbr = c.seed.copy(), c.mesh["nbr"].copy()
    seed[5], seed[6] = len(c.mesh["tri"]), -1
    got = interp.locate_walk_host(c.src_xyz, c.mesh["tri"], nbr, c.mesh["flag"], c.tgt_xyz, seed)
    others = np.ones(len(seed), dtype=bool)
    others[[5, 6]] = False
    assert (got[2][[5, 6]] == interp.MALFORMED).all() and (got[0][[5, 6]] == -1).all() and np.isnan(got[1][[5, 6]]).all()
    assert all(np.array_equal(g[others], w[others]) for g, w in zip(got, want))
    nbr[c.seed[moved]] = 2**31 - 1  # every way out of that row's first triangle
    got = interp.locate_walk_host(c.src_xyz, c.mesh["tri"], nbr, c.mesh["flag"], c.tgt_xyz, c.seed)
    assert got[2][moved] == interp.MALFORMED and got[3][moved] == 1
    same = got[2] != interp.MALFORMED
    assert same.sum() >= len(seed) - 50 and all(np.array_equal(g[same], w[same]) for g, w in zip(got, want))


# ---- the matrix ------------------------------------------------------------------------------------------------------------------
_MATRICES: dict[str, dict] = {}


def matrix_of(name):
    if name not in _MATRICES:
        c = C.case(name)
        _MATRICES[name] = interp.linear_triangulated(c.src, c.tgt)
    return _MATRICES[name]


def as_csr(m):
    return csr_array((m["matrix_data"], m["matrix_indices"], m["matrix_indptr"]), shape=tuple(int(n) for n in m["matrix_shape"]))


@pytest.mark.parametrize("name", ["O32->5deg", "random"])
def test_matrix_properties(name):
    c, m = C.case(name), matrix_of(name)
    n_tgt, n_src = len(c.tgt_xyz), len(c.src_xyz)
    assert sorted(m) == ["matrix_data", "matrix_indices", "matrix_indptr", "matrix_shape"]
    assert (m["matrix_data"].dtype, m["matrix_indices"].dtype, m["matrix_indptr"].dtype) == (np.float64, np.int32, np.int32)
    assert list(m["matrix_shape"]) == [n_tgt, n_src] and np.array_equal(m["matrix_indptr"], 3 * np.arange(n_tgt + 1))
    w, idx = m["matrix_data"].reshape(n_tgt, 3), m["matrix_indices"].reshape(n_tgt, 3)
    assert (w >= 0.0).all() and (idx >= 0).all() and (idx < n_src).all()
    assert np.abs((w[:, 0] + w[:, 1]) + w[:, 2] - 1.0).max() <= 4 * ULP
    assert np.array_equal(w, c.walked[1]) and np.array_equal(idx, c.mesh["tri"][c.walked[0]])
    point = (w[:, :, None] * c.src_xyz[idx]).sum(axis=1)  # sum w_i v_i
    direction = point / np.linalg.norm(point, axis=1, keepdims=True)
    assert np.abs(direction - c.tgt_xyz).max() <= 1e-12
    # a field that is linear in xyz is interpolated exactly: f = c . xyz gives c . (sum w_i v_i)
    coefficients = np.array([0.3, -0.5, 0.8])
    got = as_csr(m) @ (c.src_xyz @ coefficients)
    assert np.abs(got - point @ coefficients).max() <= 1e-14


@pytest.mark.parametrize("name", ["O32->5deg", "random"])
def test_a_field_regridded_onto_its_own_grid_returns_itself(name):
    c = C.self_case(name)
    m = interp.linear_triangulated(c.src, c.src)
    field = synthetic_fields(c.src, 1)[0]["values"]
    brute_tri, brute_w, brute_status = interp.locate_brute_host(c.src_xyz, c.mesh["tri"], c.mesh["flag"], c.src_xyz)
    assert (brute_status == interp.FOUND).all()
    brute_error = np.abs((brute_w * field[c.mesh["tri"][brute_tri]]).sum(axis=1) - field).max()
    tolerance = brute_error + 2 * ULP * np.abs(field).max()
    error = np.abs(as_csr(m) @ field - field).max()
    print(f"{name}: self-regrid error {error:.3e}, brute-force statement {brute_error:.3e}, tolerance {tolerance:.3e}")
    assert error <= tolerance


# ---- the mesh --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_neighbours_see_every_shared_edge_from_both_sides(name):
    c = C.case(name)
    tri, nbr = c.mesh["tri"].astype(np.int64), c.mesh["nbr"].astype(np.int64)
    assert (interp._det(*(c.src_xyz[tri[:, i]] for i in range(3))) >= 0.0).all()
    assert (interp._det(*(c.src_xyz[tri[:, i]] for i in range(3)))[c.mesh["flag"] == 0] > 0.0).all()
    assert nbr.min() >= 0 and nbr.max() < len(tri)
    for e in range(3):
        edge = np.sort(np.delete(tri, e, axis=1), axis=1)  # the edge opposite vertex e
        other = nbr[:, e]
        back = np.full(len(tri), -1)
        for f in range(3):  # the edge of the neighbour that equals `edge` is opposite its vertex f
            match = (np.sort(np.delete(tri[other], f, axis=1), axis=1) == edge).all(axis=1)
            back[match] = nbr[other[match], f]
        assert np.array_equal(back, np.arange(len(tri))), name


def test_vertex_tri_names_a_triangle_at_the_vertex_and_duplicates_get_none():
    c = C.case("2deg->5deg")
    vertex_tri, tri, hull = c.mesh["vertex_tri"], c.mesh["tri"], c.mesh["hull_vertices"]
    surplus = np.flatnonzero(vertex_tri < 0)
    assert len(surplus) == 358 and (np.abs(c.src["latitudes"][surplus]) == 90.0).all()
    assert np.array_equal(hull, np.setdiff1d(np.arange(len(vertex_tri)), surplus)) and np.array_equal(hull, np.unique(tri))
    assert (tri[vertex_tri[hull]] == hull[:, None]).any(axis=1).all()
    box = C.case("box").mesh
    for v in np.unique(box["tri"]):
        at = np.flatnonzero((box["tri"] == v).any(axis=1))
        clear = at[box["flag"][at] == 0]
        assert box["vertex_tri"][v] == (clear[0] if len(clear) else at[0])


def test_slivers_and_long_edges_are_flagged_in_the_box():
    c = C.case("box")
    v = c.src_xyz[c.mesh["tri"]]
    longest = np.sqrt(np.max([((v[:, i] - v[:, j]) ** 2).sum(axis=1) for i, j in ((1, 2), (2, 0), (0, 1))], axis=0))
    det = interp._det(v[:, 0], v[:, 1], v[:, 2])
    sliver, long_edge = det < 2.0**-20 * longest**2, longest > c.max_edge
    assert sliver.any() and long_edge.any() and np.array_equal(c.mesh["flag"] != 0, sliver | long_edge)
    assert (c.mesh["flag"] == 0).sum() >= 2 * 40 * 60  # two triangles per cell of the box, and thin ones along its curved edges
    unlimited = interp.triangulate_sphere(c.src_xyz)
    assert np.array_equal(unlimited["flag"] != 0, sliver) and np.array_equal(unlimited["tri"], c.mesh["tri"])


@pytest.mark.parametrize("points, message", [
    (np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]), "at least four"),
    (np.array([[1.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, -1.0, 0], [np.sqrt(0.5), np.sqrt(0.5), 0]]), "degenerate"),
    (np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [np.nan, 0, 0]]), "finite"),
    (np.zeros((5, 2)), "unit vectors"),
])
def test_malformed_points_raise_value_error(points, message):
    with pytest.raises(ValueError, match=message):
        interp.triangulate_sphere(points)


# ---- targets outside the domain ---------------------------------------------------------------------------------------------------
def test_outside_raises_with_the_count_or_takes_the_nearest_point():
    c = C.case("box")
    with pytest.raises(ValueError, match=r"3660 of 6161 target points lie outside .*max_edge_km.*nearest"):
        interp.linear_triangulated(c.src, c.tgt, max_edge_km=1.5 * np.pi / 180.0 * 6371.229)
    m = interp.linear_triangulated(c.src, c.tgt, max_edge_km=1.5 * np.pi / 180.0 * 6371.229, outside="nearest")
    w, idx = m["matrix_data"].reshape(-1, 3), m["matrix_indices"].reshape(-1, 3)
    found = c.brute[2] == interp.FOUND
    nearest = interp.nearest_grid_points(c.src["latitudes"], c.src["longitudes"], c.tgt["latitudes"], c.tgt["longitudes"])
    d2 = lambda i: ((c.src_xyz[i] - c.tgt_xyz) ** 2).sum(axis=1)  # noqa: E731 - cKDTree may name another of equidistant points
    assert np.array_equal(d2(idx[:, 0])[~found], d2(nearest)[~found])
    assert np.array_equal(w[~found], np.tile([1.0, 0.0, 0.0], ((~found).sum(), 1))) and (idx[~found, 1:] == idx[~found, :1]).all()
    assert np.array_equal(w[found], c.walked[1][found]) and np.array_equal(idx[found], c.mesh["tri"][c.walked[0][found]])
    assert np.array_equal(m["matrix_indptr"], 3 * np.arange(len(w) + 1))  # the matrix stays fixed-k
    with pytest.raises(ValueError, match="outside must be"):
        interp.linear_triangulated(c.src, c.tgt, outside="nan")


def test_non_finite_coordinates_raise():
    good = C.random_points(20, 5)
    bad = dict(latitudes=good["latitudes"].copy(), longitudes=good["longitudes"])
    bad["latitudes"][3] = np.inf
    for args in ((bad, good), (good, bad)):
        with pytest.raises(ValueError, match="finite"):
            interp.linear_triangulated(*args)
    with pytest.raises(ValueError, match="at least four"):
        interp.linear_triangulated({k: v[:3] for k, v in good.items()}, good)


def test_device_true_without_a_gpu_raises():
    import torch

    if not torch.cuda.is_available():  # with a GPU, tests/test_gpu_mesh_locate.py runs this call
        with pytest.raises(RuntimeError, match="device=False"):
            interp.linear_triangulated(C.random_points(20, 5), C.random_points(5, 6), device=True)


# ---- the filter ------------------------------------------------------------------------------------------------------------------
def test_filter_builds_warns_once_and_equals_the_oracle(caplog, monkeypatch):
    import torch

    if not torch.cuda.is_available():
        native_double.install(monkeypatch)
    src, tgt = C.random_points(500, 1), lookup([5.0, 5.0])
    with caplog.at_level("WARNING"):
        f = create_filter_by_name("regrid", in_grid=src, out_grid=[5.0, 5.0], method="linear-unstructured")
    plan = f.interpolator.plan
    assert type(f.interpolator).__name__ == "EarthkitRegrid" and (plan.n_src, plan.n_tgt) == (500, 2664)
    said = [r.getMessage() for r in caplog.records if "linear-unstructured" in r.getMessage()]
    assert len(said) == 1 and "unpinned" in said[0]
    specs = synthetic_fields(src, 3)
    out = list(test_source(specs) | f)
    matrix = interp.linear_triangulated(src, tgt)
    want = oracle.filter_regrid_matrix([dict(s) for s in specs], matrix={**matrix, "out_latitudes": tgt["latitudes"], "out_longitudes": tgt["longitudes"]})
    assert len(out) == 3
    for got, w_ in zip(out, want):
        assert np.array_equal(got.to_numpy(flatten=True), w_["values"])
        assert np.array_equal(got.grid_points()[0], tgt["latitudes"]) and np.array_equal(got.grid_points()[1], tgt["longitudes"])


def test_filter_takes_a_grid_name_and_an_npz_path(tmp_path):
    points = str(tmp_path / "points.npz")
    g = C.random_points(200, 9)
    np.savez(points, latitudes=g["latitudes"], longitudes=g["longitudes"])
    for in_grid, n_src in ((points, 200), ("O8", 544)):
        plan = create_filter_by_name("regrid", in_grid=in_grid, out_grid=[30.0, 30.0], method="linear-unstructured").interpolator.plan
        assert (plan.kind, plan.k, plan.n_src, plan.n_tgt) == ("ell", 3, n_src, 7 * 12)


def test_the_other_methods_keep_their_errors(tmp_path):
    src = C.random_points(200, 9)
    for method in (None, "linear"):
        with pytest.raises(NotImplementedError, match="matrix"):
            create_filter_by_name("regrid", in_grid=src, out_grid=[30.0, 30.0], method=method)
    with pytest.raises(NotImplementedError, match="matrix"):
        create_filter_by_name("regrid", in_grid="o32", out_grid="o48", method="conservative")


# ---- the command -----------------------------------------------------------------------------------------------------------------
def test_cli_file_round_trips_through_the_filter(tmp_path):
    source, target, path = str(tmp_path / "lam.npz"), str(tmp_path / "targets.npz"), str(tmp_path / "m.npz")
    c = C.case("box")
    np.savez(source, **c.src)
    np.savez(target, **c.tgt)
    with pytest.raises(SystemExit, match="3660 of 6161"):
        cli.main(["make-regrid-file", "linear-matrix", source, target, "--max-edge-km", "170", "--output", path])
    assert cli.main(["make-regrid-file", "linear-matrix", source, target, "--max-edge-km", "170", "--outside", "nearest", "--output", path]) == 0
    loaded = interp.load_matrix_npz(path)
    assert sorted(loaded) == ["in_latitudes", "in_longitudes", "matrix_data", "matrix_indices", "matrix_indptr", "matrix_shape",
                              "out_latitudes", "out_longitudes"]
    want = interp.linear_triangulated(c.src, c.tgt, max_edge_km=170.0, outside="nearest")
    assert all(np.array_equal(loaded[k], want[k]) for k in want)
    assert np.array_equal(loaded["in_latitudes"], c.src["latitudes"]) and np.array_equal(loaded["out_longitudes"], c.tgt["longitudes"])
    plan = create_filter_by_name("regrid", matrix=path).interpolator.plan  # the file is what regrid(matrix=...) reads
    assert (plan.kind, plan.k, plan.n_src, plan.n_tgt) == ("ell", 3, 2501, 6161)


# ---- the C ABI of the companion library ------------------------------------------------------------------------------------------
def header_declarations() -> list[str]:
    return abi_checks.header_declarations(HEADER, "ATX_MESH_API")


def test_header_declares_the_binding():
    text = open(HEADER).read()
    assert header_declarations() == ["atx_mesh_version", "atx_mesh_last_error", "atx_mesh_locate"]
    assert sorted(native_mesh.SIGNATURES) == sorted(header_declarations())
    assert re.search(r"#define ATX_MESH_VERSION 420\b", text) and '#include "atx.h"' in text
    assert re.search(r"#define ATX_MESH_MAX_STEPS (\d+)\b", text).group(1) == str(native_mesh.MAX_STEPS)
    declared = re.search(r"atx_mesh_locate\(([^)]*)\);", text).group(1)
    assert len(declared.split(",")) == 15 == len(native_mesh.SIGNATURES["atx_mesh_locate"][1])


def test_header_is_plain_c99(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "use_header.c"
    src.write_text('#include "atx_mesh.h"\nint use(void) { return ATX_MESH_VERSION + ATX_MESH_MAX_STEPS + ATX_OK + ATX_EINVAL; }\n')
    run = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "use_header.o")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


def malformed_calls():
    """(arguments, word of the message) for every argument check of atx_mesh_locate: nothing is launched, no pointer is read."""
    import ctypes

    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    good = [one, 500, one, one, one, 996, one, one, 10, 64, one, one, one, one, None]
    for pos, bad, word in ((1, 0, b"n_src"), (1, 2**31, b"n_src"), (5, 0, b"n_tri"), (5, -1, b"n_tri"), (5, 2**31, b"n_tri"),
                           (8, -1, b"n_tgt"), (8, 2**31, b"n_tgt"), (9, -1, b"max_steps"), (9, native_mesh.MAX_STEPS + 1, b"max_steps")):
        yield good[:pos] + [bad] + good[pos + 1:], word
    for pos in (0, 2, 3, 4, 6, 7, 10, 11, 12, 13):
        yield good[:pos] + [None] + good[pos + 1:], b"null"


def test_abi_argument_validation_without_a_gpu():
    if not os.path.exists(native_mesh.lib_path()):
        pytest.skip("libatx_mesh.so is not built")
    lib = native_mesh.load()
    assert lib.atx_mesh_version() == 420
    n = 0
    for args, word in malformed_calls():
        assert lib.atx_mesh_locate(*args) == native_mesh.EINVAL and word in lib.atx_mesh_last_error(), (args, lib.atx_mesh_last_error())
        n += 1
    assert n == 9 + 10
    # no targets: nothing launched, no storage needed ... but the rest is still validated
    nothing = [None, 500, None, None, None, 996, None, None, 0, 64, None, None, None, None, None]
    assert lib.atx_mesh_locate(*nothing) == native_mesh.OK
    for pos, bad in ((1, 0), (5, 0), (9, -1)):
        assert lib.atx_mesh_locate(*(nothing[:pos] + [bad] + nothing[pos + 1:])) == native_mesh.EINVAL
