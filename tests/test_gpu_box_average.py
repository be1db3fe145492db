"""Grid-box-average regridding on the device: ``atx_plan_box_average_count`` / ``_fill`` against the host statement bit for bit (small
pairs, several workgroups, past the grid cap), their argument checks, and ``regrid(method="grid-box-average")`` end to end — float64
against scipy's CSR product of the statement bit for bit, float32 within ``smoke()``'s bound, conservation of the area-weighted mean,
fused against filter by filter — and ``method="nearest-neighbour"`` against ``method="nearest"``.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch
from scipy.sparse import csr_array

import box_average_restatement as R
from anemoi_transform_amd import interp, native_plan
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.grids import lookup
from test_box_average_host import malformed_calls
from test_filters import test_source

pytestmark = pytest.mark.gpu

LARGER = {
    "O32->5deg": ("O32", [5.0, 5.0]),  # 2 664 targets: several workgroups
    "10deg->0.25x0.4deg": ([10.0, 10.0], [0.25, 0.4]),  # 648 900 targets, past the 2048 x 256 cap; rows of 1-2 entries
}
_HOST: dict[str, dict] = {}


def pair(name):
    src, tgt = {**R.PAIRS, **R.IDENTITIES, **LARGER}[name]
    return R.rows_of(src), R.rows_of(tgt)


def host(name):
    if name not in _HOST:
        _HOST[name] = interp.box_average_rows(*pair(name), device=False)
    return _HOST[name]


def device_tables(name, dev):
    return [native_plan.RowTable(*(torch.from_numpy(a).to(dev) for a in interp.box_row_table(rows)), n_points=int(np.sum(rows[1])))
            for rows in pair(name)]


@pytest.mark.parametrize("name", list(R.PAIRS) + list(R.IDENTITIES) + list(LARGER))
def test_device_equals_host_bit_for_bit(dev, name):
    got = interp.box_average_rows(*pair(name), device=True)
    R.check_equal(got, host(name), name)
    if name in R.PAIRS or name in R.IDENTITIES:
        R.check_equal(got, R.statement(name), name + " against the restatement")


def test_past_the_cap_pair_is_past_the_cap():
    n_tgt, lengths = int(host("10deg->0.25x0.4deg")["matrix_shape"][0]), np.diff(host("10deg->0.25x0.4deg")["matrix_indptr"])
    assert n_tgt == 648900 > 2048 * 256 and (lengths.min(), lengths.max()) == (1, 2)
    assert int(host("O32->5deg")["matrix_shape"][0]) == 2664


@pytest.mark.parametrize("name", ["O16->O4", "30deg->O8", "7.2deg->36deg", "O32->5deg", "10deg->0.25x0.4deg"])
def test_count_kernel_gives_the_row_lengths(dev, name):
    src, tgt = device_tables(name, dev)
    count = torch.full((tgt.n_points,), -7, dtype=torch.int64, device=dev)
    native_plan.box_average_count(src, tgt, count)
    assert np.array_equal(count.cpu().numpy(), np.diff(host(name)["matrix_indptr"].astype(np.int64)))


def test_malformed_calls_are_rejected_without_a_launch(dev):
    """Every malformed call of tests/test_box_average_host.py, here with real buffers behind the pointers that are not under test:
    the status is ATX_EINVAL and no byte of the outputs changes."""
    lib = native_plan.load()
    src, tgt = device_tables("O16->O4", dev)
    m = host("O16->O4")
    nnz = len(m["matrix_indices"])
    count = torch.full((tgt.n_points,), -7, dtype=torch.int64, device=dev)
    indptr = torch.from_numpy(m["matrix_indptr"]).to(dev)
    indices = torch.full((nnz,), -7, dtype=torch.int32, device=dev)
    data = torch.full((nnz,), -7.0, dtype=torch.float64, device=dev)
    real = {"count": [*src.args(), *tgt.args(), count.data_ptr(), None],
            "fill": [*src.args(), *tgt.args(), indptr.data_ptr(), nnz, indices.data_ptr(), data.data_ptr(), None]}
    placeholder = ctypes.c_void_p(16).value
    n = 0
    for call, args, word in malformed_calls(lib):
        kind = "count" if len(args) == 12 else "fill"
        sent = [r if (isinstance(a, ctypes.c_void_p) and a.value == placeholder) or (a == 30 and kind == "fill" and i == 11) else a
                for i, (a, r) in enumerate(zip(args, real[kind]))]
        assert call(*sent) == native_plan.EINVAL and word in lib.atx_plan_last_error(), (kind, args)
        n += 1
    assert n == 32
    torch.cuda.synchronize()
    assert bool((count == -7).all()) and bool((indices == -7).all()) and bool((data == -7.0).all())
    # the binding refuses tensors of the wrong kind before the library sees them
    with pytest.raises(ValueError, match="count"):
        native_plan.box_average_count(src, tgt, count[:-1])
    with pytest.raises(ValueError, match="indptr"):
        native_plan.box_average_fill(src, tgt, indptr.to(torch.int64), indices, data)
    with pytest.raises(ValueError, match="indptr"):
        native_plan.box_average_fill(src, tgt, indptr, indices, data.to(torch.float32))
    with pytest.raises(ValueError, match="HBM"):
        native_plan.RowTable(src.z.cpu(), src.len, src.start, n_points=src.n_points)


def fields_on(grid, n_lev, np_dtype, seed=20260630):
    rng = np.random.default_rng(seed)
    n = len(grid["latitudes"])
    return [{"param": "t", "levelist": l + 1, "values": (280.0 + 30.0 * rng.standard_normal(n)).astype(np_dtype),
             "latitudes": grid["latitudes"], "longitudes": grid["longitudes"], "valid_datetime": "2020-01-01T00:00:00Z"} for l in range(n_lev)]


FILTER_PAIRS = {"O16->O4": ("O16", "O4"), "10deg->O8": ([10.0, 10.0], "O8")}


def statement_csr(name):
    src, tgt = FILTER_PAIRS[name]
    m = interp.box_average_rows(R.rows_of(src), R.rows_of(tgt), device=False)
    return csr_array((m["matrix_data"], m["matrix_indices"], m["matrix_indptr"]), shape=tuple(int(n) for n in m["matrix_shape"]))


@pytest.mark.parametrize("name", sorted(FILTER_PAIRS))
@pytest.mark.parametrize("np_dtype", [np.float64, np.float32])
def test_filter_end_to_end(dev, name, np_dtype):
    src, tgt = FILTER_PAIRS[name]
    specs = fields_on(lookup(src), 3, np_dtype)
    out = list(test_source(specs) | create_filter_by_name("regrid", in_grid=src, out_grid=tgt, method="grid-box-average"))
    matrix = statement_csr(name)
    assert len(out) == 3
    for field, spec in zip(out, specs):
        got = field.to_numpy(flatten=True)
        assert np.array_equal(field.grid_points()[0], lookup(tgt)["latitudes"])
        if np_dtype == np.float64:
            assert got.dtype == np.float64 and np.array_equal(got, matrix @ spec["values"]), "not scipy's CSR product bit for bit"
        else:
            np.testing.assert_allclose(got, matrix @ spec["values"].astype(np.float64), rtol=1e-6)


@pytest.mark.parametrize("name", sorted(FILTER_PAIRS))
def test_the_area_weighted_mean_is_conserved(dev, name):
    src, tgt = FILTER_PAIRS[name]
    specs = fields_on(lookup(src), 3, np.float64, seed=7)
    out = list(test_source(specs) | create_filter_by_name("regrid", in_grid=src, out_grid=tgt, method="grid-box-average"))
    src_area, tgt_area = R.cell_areas(R.rows_of(src)), R.cell_areas(R.rows_of(tgt))
    assert len(src_area) <= 1600
    for field, spec in zip(out, specs):
        before, after = float(np.sum(src_area * spec["values"])), float(np.sum(tgt_area * field.to_numpy(flatten=True)))
        print(f"{name}: mean {before!r} -> {after!r}, relative {abs(after - before) / before:.3e}")
        assert abs(after - before) <= 1e-12 * before


def test_fused_equals_filter_by_filter(dev, monkeypatch):
    specs = fields_on(lookup("O16"), 3, np.float64)

    def run():
        return list(test_source(specs) | create_filter_by_name("regrid", in_grid="O16", out_grid="O4", method="grid-box-average")
                    | create_filter_by_name("rescale", scale=1.0, offset=-273.15, param="t"))

    fused = run()
    monkeypatch.setenv("ATX_NO_FUSION", "1")
    stepwise = run()
    matrix = statement_csr("O16->O4")
    assert len(fused) == len(stepwise) == 3
    for a, b, spec in zip(fused, stepwise, specs):
        assert np.array_equal(a.to_numpy(flatten=True), b.to_numpy(flatten=True))
        assert np.array_equal(a.to_numpy(flatten=True), (matrix @ spec["values"]) * 1.0 + -273.15)


def test_nearest_neighbour_equals_nearest(dev):
    specs = fields_on(lookup("O8"), 3, np.float64)
    a = list(test_source(specs) | create_filter_by_name("regrid", in_grid="O8", out_grid=[30.0, 30.0], method="nearest-neighbour"))
    b = list(test_source(specs) | create_filter_by_name("regrid", in_grid="O8", out_grid=[30.0, 30.0], method="nearest"))
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert np.array_equal(x.to_numpy(flatten=True), y.to_numpy(flatten=True))
        assert np.array_equal(x.grid_points()[1], y.grid_points()[1])
