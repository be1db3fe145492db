"""The k-NN, cutout and superob kernels (``atx_knn_build``, ``atx_knn_query``, ``atx_cutout_inside``, ``atx_obs_group_mean``,
``atx_obs_group_argmin``) driven directly on the device and held to exact host statements by the checks of
tests/knn_superob_checks.py: every ``knn_query_kernel<K>`` instance, source sizes around the leaf and the padded tree, point sets
chosen to tie, a reused workspace, canaries around every buffer, the build loops past the workgroup cap; triangles of the test's own
choosing with points on vertices and edges, ``a`` next to ±1e-7 and stray neighbour indices; group lengths around the unroll, a
wave and kLongGroup, long groups in chosen lanes, pitched inputs and outputs, special values, the minimum walked through every
position, and the guards for bad bounds and row indices.  tests/test_knn_superob_checks_catch_defects.py shows each named case
failing on a planted defect."""

from __future__ import annotations

import time

import pytest

import knn_superob_checks as C
from anemoi_transform_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kern():
    return C.Kernels(knn_build=native.KnnIndex, knn_workspace_bytes=lambda n: native.load().atx_knn_workspace_bytes(n),
                     cutout_inside=native.cutout_inside, group_mean=native.obs_group_mean, group_argmin=native.obs_group_argmin)


# ---- k-NN -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", C.knn_every_k())
def test_knn_every_template_instance(dev, kern, k):
    C.check_knn_every_k(kern, dev, ks=[k])


@pytest.mark.parametrize("n_src", C.knn_source_sizes())
def test_knn_source_sizes_around_the_leaf_and_the_padded_tree(dev, kern, n_src):
    C.check_knn_source_size(kern, dev, n_src)


@pytest.mark.parametrize("n_tgt", C.knn_target_counts())
def test_knn_target_counts(dev, kern, n_tgt):
    C.check_knn_target_count(kern, dev, n_tgt)


@pytest.mark.parametrize("name", C.tie_sets())
def test_knn_orders_exact_ties_by_source_index(dev, kern, name):
    C.check_knn_ties(kern, dev, name)


def test_knn_workspace_reused_for_a_smaller_index(dev, kern):
    C.check_knn_reuse(kern, dev)


def test_knn_writes_nothing_outside_its_buffers(dev, kern):
    C.check_knn_buffers(kern, dev)


def test_knn_build_loops_past_the_workgroup_cap(dev, kern):
    """The one case allowed to run longer: 16 * 2^20 + 9 sources, the brute force on the host included."""
    t0 = time.perf_counter()
    sizes = C.check_knn_past_the_cap(kern, dev)
    assert sizes["padded leaves"] == 4 * sizes["sweep"] and sizes["workspace bytes"] < 2 << 30
    print(f"past the cap: {sizes}, {time.perf_counter() - t0:.1f} s")


# ---- cutout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", C.CUTOUT_SHAPES)
def test_cutout_on_neighbour_tables_of_a_jittered_patch(dev, kern, k, n):
    C.check_cutout_patch(kern, dev, k, n)


def test_cutout_points_on_vertices_and_edges(dev, kern):
    C.check_cutout_constructed(kern, dev)


def test_cutout_points_on_the_edges_of_a_regular_patch(dev, kern):
    C.check_cutout_edge_points(kern, dev)


def test_cutout_a_next_to_epsilon(dev, kern):
    C.check_cutout_epsilon(kern, dev)


def test_cutout_skips_stray_neighbour_indices(dev, kern):
    C.check_cutout_stray(kern, dev)


# ---- superob --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", (False, True), ids=("in-order", "shuffled"))
def test_group_mean_and_argmin_at_every_edge_length(dev, kern, shuffled):
    C.check_mean_edge_lengths(kern, dev, shuffled)


@pytest.mark.parametrize("name", C.group_count_cases())
def test_group_mean_and_argmin_group_counts_and_long_groups_by_lane(dev, kern, name):
    C.check_mean_group_counts(kern, dev, name)


def test_group_mean_special_values(dev, kern):
    C.check_mean_special_values(kern, dev)


@pytest.mark.parametrize("length", (C.K.long_group + C.K.wave + 1, C.K.long_group))
def test_group_argmin_minimum_walked_through_every_position(dev, kern, length):
    C.check_argmin_walk(kern, dev, length)


def test_group_argmin_edge_groups(dev, kern):
    C.check_argmin_edge_groups(kern, dev)


def test_superob_guards_on_bad_bounds_and_row_indices(dev, kern):
    C.check_superob_guards(kern, dev)
