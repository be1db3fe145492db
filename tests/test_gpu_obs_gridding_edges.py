"""The observation gridding kernels (``atx_obs_best_per_cell``, ``atx_obs_fill_stack``) driven directly on the device and held to an
exact loop by the checks of tests/obs_gridding_checks.py: row counts around a wave and a workgroup with the winner walked through
the blocks' first and last lanes, pairs of rows whose scores are equal as real numbers (so that a contracted or reciprocal rounding
changes a winner), every window closure a nanosecond either side of its ends, differences past 2^53 ns, rows and targets that take
no part, pitched values, stray cells beside other targets' slots, the refusals; then the fill from handmade winner tables: both
layouts at every pitch and alignment route, the levels of the COLUMNS layout, target counts around the ``grid.y`` cap, stray winners,
value bit patterns and empty stacks — every table and stack between canaries.  tests/test_obs_gridding_checks_catch_defects.py shows
each named case failing on a planted defect."""

from __future__ import annotations

import time

import pytest

import obs_gridding_checks as C
from anemoi_transform_amd import native

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("layout", (C.FIELDS, C.COLUMNS), ids=("fields", "columns"))


@pytest.fixture(scope="module")
def kern():
    t0 = time.perf_counter()
    yield C.Kernels(best_per_cell=native.obs_best_per_cell, fill_stack=native.obs_fill_stack)
    print(f"\ntests/test_gpu_obs_gridding_edges.py: {time.perf_counter() - t0:.1f} s")


# ---- atx_obs_best_per_cell ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.row_counts())
def test_best_row_counts_and_the_winner_walked_through_the_blocks(dev, kern, n):
    C.check_best_row_count(kern, dev, n)


@pytest.mark.parametrize("n_cols", C.ROUNDING_COLUMNS)
def test_best_pairs_of_equal_real_scores_keep_the_two_roundings(dev, kern, n_cols):
    C.check_best_rounding(kern, dev, n_cols)


@pytest.mark.parametrize("name", C.weight_tables())
def test_best_weights_one_zero_and_the_smallest(dev, kern, name):
    C.check_best_weight(kern, dev, name)


@pytest.mark.parametrize("name", C.window_tables())
def test_best_window_ends(dev, kern, name):
    C.check_best_window(kern, dev, name)


def test_best_differences_past_2_to_the_53(dev, kern):
    C.check_best_big_difference(kern, dev)


@pytest.mark.parametrize("name", C.absent_tables())
def test_best_rows_that_never_take_part(dev, kern, name):
    C.check_best_absent(kern, dev, name)


@pytest.mark.parametrize("name", C.target_tables())
def test_best_targets(dev, kern, name):
    C.check_best_targets(kern, dev, name)


@pytest.mark.parametrize("name", C.pitched_tables())
def test_best_pitched_values(dev, kern, name):
    C.check_best_pitched(kern, dev, name)


def test_best_stray_cells_stay_out_of_other_slots(dev, kern):
    C.check_best_stray_cells(kern, dev)


@pytest.mark.parametrize("name", C.refusal_calls())
def test_best_refusals_touch_nothing(dev, kern, name):
    C.check_best_refusal(kern, dev, name)


# ---- atx_obs_fill_stack ---------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("n_cells", C.fill_cell_counts())
def test_fill_layouts_pitches_and_alignment(dev, kern, layout, n_cells):
    C.check_fill_layout(kern, dev, layout, n_cells)


@pytest.mark.parametrize("n_time,n_cols", C.COLUMN_SHAPES)
def test_fill_levels_of_the_columns_layout(dev, kern, n_time, n_cols):
    C.check_fill_columns_levels(kern, dev, n_time, n_cols)


@pytest.mark.parametrize("n_time", C.fill_target_counts())
def test_fill_fields_targets_around_the_grid_y_cap(dev, kern, n_time):
    C.check_fill_many_targets(kern, dev, n_time)


def test_both_kernels_end_to_end_past_the_grid_y_cap(dev, kern):
    C.check_end_to_end_many_targets(kern, dev)


@LAYOUTS
def test_fill_stray_winners_give_nan_in_both_layouts(dev, kern, layout):
    C.check_fill_stray_winners(kern, dev, layout)


@LAYOUTS
def test_fill_copies_value_bit_patterns(dev, kern, layout):
    C.check_fill_bit_patterns(kern, dev, layout)


@LAYOUTS
def test_fill_empty_table_no_levels_no_points(dev, kern, layout):
    C.check_fill_nothing(kern, dev, layout)
