"""Point location on the device: ``atx_mesh_locate`` against ``interp.locate_walk_host`` bit for bit on the point sets of
tests/linear_unstructured_cases.py (partial and full waves, bounded walks, planted out-of-range seeds and neighbours),
``interp.linear_triangulated(device=True)`` against ``device=False``, and ``regrid(method="linear-unstructured")`` on resident
float64 and float32 stacks against the oracle's CSR statement of the host-built matrix.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import linear_unstructured_cases as C
from anemoi_transform_amd import interp, native_mesh
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.grids import lookup
from oracle import oracle
from test_filters import synthetic_fields, test_source
from test_linear_unstructured_host import malformed_calls

pytestmark = pytest.mark.gpu

NAMES = ("tri_out", "w", "status", "steps")


def on_device(c, dev, tri=None, nbr=None):
    mesh = c.mesh
    return native_mesh.Mesh(torch.from_numpy(c.src_xyz).to(dev), torch.from_numpy(mesh["tri"] if tri is None else tri).to(dev),
                            torch.from_numpy(mesh["nbr"] if nbr is None else nbr).to(dev), torch.from_numpy(mesh["flag"]).to(dev))


def locate(c, dev, *, rows=slice(None), seed=None, max_steps=64, **tables):
    seed = c.seed[rows] if seed is None else seed
    got = native_mesh.locate(on_device(c, dev, **tables), torch.from_numpy(np.ascontiguousarray(c.tgt_xyz[rows])).to(dev),
                             torch.from_numpy(np.ascontiguousarray(seed)).to(dev), max_steps)
    return [t.cpu().numpy() for t in got]


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_kernel_equals_the_host_walk_bit_for_bit(dev, name):
    c = C.case(name)
    got = locate(c, dev)
    print(f"{name}: status counts {np.bincount(got[2], minlength=4)}, at most {got[3].max()} moves")
    for label, g, want in zip(NAMES, got, c.walked):
        assert g.dtype == want.dtype and np.array_equal(g, want), (name, label)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2664])
def test_partial_and_full_waves(dev, n):
    c = C.case("O32->5deg")
    rows = slice(2664 - n, 2664)  # the last rows: the walk moves there too
    got = locate(c, dev, rows=rows)
    for label, g, want in zip(NAMES, got, c.walked):
        assert g.shape == want[rows].shape and np.array_equal(g, want[rows]), (n, label)


@pytest.mark.parametrize("max_steps", [0, 2])
def test_a_bounded_walk_leaves_rows_undecided_and_the_matrix_is_the_same(dev, max_steps):
    c = C.case("O32->5deg")
    got, want = locate(c, dev, max_steps=max_steps), c.walk(max_steps)
    assert (want[2] == interp.UNDECIDED).any() and want[3].max() == max_steps
    for label, g, w in zip(NAMES, got, want):
        assert np.array_equal(g, w), (max_steps, label)
    full = interp.linear_triangulated(c.src, c.tgt, device=True)
    bounded = interp.linear_triangulated(c.src, c.tgt, device=True, max_steps=max_steps)
    assert all(np.array_equal(bounded[k], full[k]) for k in full)


def test_planted_out_of_range_entries_end_their_rows_alone(dev):
    c = C.case("random")
    want = c.walked
    n_tri = len(c.mesh["tri"])
    seed = c.seed.copy()
    seed[[5, 6, 1999]] = n_tri, -1, 2**31 - 1
    got = locate(c, dev, seed=seed)
    planted = np.zeros(len(seed), dtype=bool)
    planted[[5, 6, 1999]] = True
    assert (got[2][planted] == native_mesh.MALFORMED).all() and (got[0][planted] == -1).all() and np.isnan(got[1][planted]).all()
    assert (got[3][planted] == 0).all() and all(np.array_equal(g[~planted], w[~planted]) for g, w in zip(got, want))

    moved = int(np.flatnonzero(want[3] > 0)[0])
    nbr = c.mesh["nbr"].copy()
    nbr[c.seed[moved]] = n_tri, -7, 2**31 - 1  # every way out of that row's first triangle
    got = locate(c, dev, nbr=nbr)
    host = interp.locate_walk_host(c.src_xyz, c.mesh["tri"], nbr, c.mesh["flag"], c.tgt_xyz, c.seed)
    assert got[2][moved] == native_mesh.MALFORMED and got[3][moved] == 1 and np.isnan(got[1][moved]).all()
    assert all(np.array_equal(g, h, equal_nan=True) for g, h in zip(got, host))
    same = got[2] != native_mesh.MALFORMED
    assert same.sum() >= len(seed) - 50 and all(np.array_equal(g[same], w[same]) for g, w in zip(got, want))

    tri = c.mesh["tri"].copy()
    tri[c.seed[moved]] = len(c.src_xyz), 0, 1  # a vertex past the source points
    got = locate(c, dev, tri=tri)
    host = interp.locate_walk_host(c.src_xyz, tri, c.mesh["nbr"], c.mesh["flag"], c.tgt_xyz, c.seed)
    assert got[2][moved] == native_mesh.MALFORMED and got[3][moved] == 0
    assert all(np.array_equal(g, h, equal_nan=True) for g, h in zip(got, host))


def test_malformed_calls_are_rejected_without_a_launch(dev):
    """Every malformed call of tests/test_linear_unstructured_host.py, here with real buffers behind the pointers that are not under
    test: the status is ATX_EINVAL and no byte of the outputs changes."""
    import ctypes

    lib = native_mesh.load()
    c = C.case("random")
    mesh = on_device(c, dev)
    n = 10
    tgt, seed = torch.from_numpy(c.tgt_xyz[:n].copy()).to(dev), torch.from_numpy(c.seed[:n].copy()).to(dev)
    tri_out = torch.full((n,), -7, dtype=torch.int32, device=dev)
    w = torch.full((n, 3), -7.0, dtype=torch.float64, device=dev)
    status, steps = tri_out.clone(), tri_out.clone()
    real = [mesh.src_xyz.data_ptr(), mesh.n_src, mesh.tri.data_ptr(), mesh.nbr.data_ptr(), mesh.flag.data_ptr(), mesh.n_tri, tgt.data_ptr(),
            seed.data_ptr(), n, 64, tri_out.data_ptr(), w.data_ptr(), status.data_ptr(), steps.data_ptr(), None]
    count = 0
    for args, word in malformed_calls():
        sent = [r if isinstance(a, ctypes.c_void_p) else a for a, r in zip(args, real)]
        assert lib.atx_mesh_locate(*sent) == native_mesh.EINVAL and word in lib.atx_mesh_last_error(), args
        count += 1
    assert count == 19
    torch.cuda.synchronize()
    assert bool((tri_out == -7).all()) and bool((w == -7.0).all()) and bool((status == -7).all()) and bool((steps == -7).all())
    # the binding refuses tensors of the wrong kind before the library sees them
    with pytest.raises(ValueError, match="seed"):
        native_mesh.locate(mesh, tgt, seed.to(torch.int64))
    with pytest.raises(ValueError, match="tgt_xyz"):
        native_mesh.locate(mesh, tgt.cpu(), seed)
    with pytest.raises(ValueError, match="max_steps"):
        native_mesh.locate(mesh, tgt, seed, -1)
    with pytest.raises(ValueError, match="tri"):
        native_mesh.Mesh(mesh.src_xyz, mesh.tri.to(torch.int64), mesh.nbr, mesh.flag)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_device_matrix_equals_host_matrix(dev, name):
    c = C.case(name)
    kwargs = {} if c.max_edge is None else dict(max_edge_km=2.0 * np.arcsin(c.max_edge / 2.0) * 6371.229 + 1.0, outside="nearest")
    host = interp.linear_triangulated(c.src, c.tgt, device=False, **kwargs)
    got = interp.linear_triangulated(c.src, c.tgt, device=True, **kwargs)
    assert np.array_equal(got["matrix_indptr"], host["matrix_indptr"]) and np.array_equal(got["matrix_indices"], host["matrix_indices"])
    assert got["matrix_data"].dtype == np.float64 and np.array_equal(got["matrix_data"], host["matrix_data"])
    assert np.array_equal(got["matrix_shape"], host["matrix_shape"])


@pytest.mark.parametrize("np_dtype", [np.float64, np.float32])
def test_filter_on_resident_stacks_equals_the_oracle(dev, np_dtype):
    src, tgt = C.random_points(500, 1), lookup([5.0, 5.0])
    specs = synthetic_fields(src, 4)
    for s in specs:
        s["values"] = s["values"].astype(np_dtype)
    out = list(test_source(specs) | create_filter_by_name("regrid", in_grid=src, out_grid=[5.0, 5.0], method="linear-unstructured"))
    matrix = interp.linear_triangulated(src, tgt, device=False)
    want = oracle.filter_regrid_matrix([dict(s) for s in specs], matrix={**matrix, "out_latitudes": tgt["latitudes"], "out_longitudes": tgt["longitudes"]})
    assert len(out) == 4
    for field, w_ in zip(out, want):
        got = field.to_numpy(flatten=True)
        assert np.array_equal(field.grid_points()[0], tgt["latitudes"])
        if np_dtype == np.float64:
            assert got.dtype == np.float64 and np.array_equal(got, w_["values"]), "not the oracle's CSR statement bit for bit"
        else:
            np.testing.assert_allclose(got, np.asarray(w_["values"], dtype=np.float64), rtol=1e-6)
