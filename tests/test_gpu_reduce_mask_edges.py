"""The reduction and mask kernels (``atx_reduce``, ``atx_reduce_stack``, ``atx_mask_build``, ``atx_mask_count``, ``atx_mask_to_index``),
the index guard ``atx_check_indices`` and ``atx_stream_copy`` on the device, held to numpy by the checks of
tests/reduce_mask_checks.py: an extreme and a NaN walked through every structurally distinct position of every storage shape, special
values, both finishing routes, every route past the workgroup cap, every comparison against every awkward threshold, masks of any
non-zero bytes, canaries behind everything written.  tests/test_reduce_mask_checks_catch_defects.py shows each check failing on a
planted defect."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import reduce_mask_checks as C
from anemoi_transform_amd import native

pytestmark = pytest.mark.gpu


def index_into(mask, n, index):
    """``atx_mask_to_index`` into the caller's buffer; returns the count."""
    workspace = torch.empty(max(native.load().atx_mask_to_index_workspace(n), 16), dtype=torch.uint8, device=index.device)
    count = torch.full((1,), -7, dtype=torch.int64, device=index.device)
    native._call("atx_mask_to_index", native._ptr(mask), n, native._ptr(index), native._ptr(count), native._ptr(workspace),
                 workspace.numel(), native._stream())
    return int(count.item())


@pytest.fixture
def kern(monkeypatch):
    return C.Kernels(reduce=native.reduce, reduce_stack=native.reduce_stack, mask_build=native.mask_build, mask_count=native.mask_count,
                     mask_to_index=native.mask_to_index, index_into=index_into, check_indices=native.check_indices,
                     stream_copy=native.stream_copy, use_workspace=lambda flag: monkeypatch.setattr(native, "_REDUCE_TICKET", flag))


SMALL = [s for dt in C.DTYPES for s in C.small_shapes(dt)]
LARGER = [s for dt in C.DTYPES for s in C.mid_shapes(dt) + C.flat_shapes(dt)]
# special values on one shape of every kind of storage and route
SPECIAL = [s for s in SMALL if "-len5-" in s.name or "-len8-odd" in s.name] + LARGER


@pytest.mark.parametrize("shape", SMALL + LARGER, ids=lambda s: f"{s.name}-{s.route()}")
def test_an_extreme_and_a_nan_walked_through_every_position(dev, kern, shape):
    assert C.check_walked_positions(kern, dev, shape) > 0


@pytest.mark.parametrize("shape", SPECIAL, ids=lambda s: f"{s.name}-{s.route()}")
def test_special_values(dev, kern, shape):
    C.check_special_values(kern, dev, shape)


@pytest.mark.parametrize("shape,host_copy", C.past_cap_shapes(), ids=lambda v: f"{v.name}-{v.route()}" if isinstance(v, C.Shape) else str(v))
def test_every_route_past_the_workgroup_cap(dev, kern, shape, host_copy):
    sizes = C.check_past_the_cap(kern, dev, shape, host_copy=host_copy)
    assert sizes["items"] > 2 * sizes["threshold"] and sizes["bytes"] < 4 << 30
    print(f"past the cap: {sizes}")


@pytest.mark.parametrize("threshold", C.THRESHOLDS, ids=repr)
@pytest.mark.parametrize("np_dtype", C.DTYPES, ids=["f32", "f64"])
def test_mask_build_every_comparison(dev, kern, np_dtype, threshold):
    C.check_mask_build(kern, dev, np_dtype, threshold)


@pytest.mark.parametrize("np_dtype", C.DTYPES, ids=["f32", "f64"])
def test_mask_build_past_the_grid_cap(dev, kern, np_dtype):
    assert C.check_mask_build_past_the_cap(kern, dev, np_dtype) > C.K.stream_grid * C.K.block * 4


@pytest.mark.parametrize("density", C.DENSITIES)
@pytest.mark.parametrize("n", C.index_lengths())
def test_mask_count_and_index_of_any_non_zero_bytes(dev, kern, n, density):
    C.check_mask_count_and_index(kern, dev, n, density)


@pytest.mark.parametrize("n", C.check_indices_lengths())
def test_check_indices_counts_what_numpy_counts(dev, kern, n):
    C.check_check_indices(kern, dev, n)


@pytest.mark.parametrize("n_bytes", C.stream_copy_sizes())
def test_stream_copy_is_a_bit_copy(dev, kern, n_bytes):
    C.check_stream_copy(kern, dev, n_bytes)
