"""The comparison that tests/test_obs_qc_host.py and tests/test_gpu_obs_qc.py rest on — interpret the compiled launches, compare with
the plain numpy statement on bit patterns — must FAIL when the thing under test is wrong.  Five defects are injected into the
interpreter (which stands for the kernel) or into the statement, and the recorded cases must catch each of them."""

from __future__ import annotations

import numpy as np
import pytest

import row_program_restatement as R
from test_obs_qc_host import GOLDEN, agree, case_table, interpreted

CASES = GOLDEN["cases"]


def caught(**defect) -> list[str]:
    """The recorded cases on which the defective interpreter no longer gives the statement."""
    out = []
    for case in CASES:
        table = case_table(case)
        if not agree(interpreted(case["filter"], case["config"], table, **defect), R.statement(case["filter"], case["config"], table)):
            out.append(case["id"])
    return out


def test_the_sound_interpreter_passes_every_case():
    assert caught() == []


@pytest.mark.parametrize("defect, filters", [("ge_as_gt", {"mask_tabular", "exclude_dates"}),
                                             ("nan_where_inverted", {"mask_tabular", "mask_outside_range", "mask_infs", "mask_dewpoint_temperature",
                                                                     "exclude_dates", "remove_extreme_values"}),
                                             ("y_from_two_back", {"mask_outside_range", "exclude_dates", "clip_tabular", "drop_nans_tabular"})])
def test_a_defective_kernel_is_caught(defect, filters):
    assert defect in R.DEFECTS
    found = caught(defect=defect)
    assert filters <= {case["filter"] for case in CASES if case["id"] in found}, found
    assert any(i.startswith("reference_") for i in found) and any(i.startswith("seeded_") for i in found)


def test_scalars_that_are_not_rounded_for_float32_are_caught():
    found = caught(dtypes_as_float64=True)  # the compiler is told every column is float64: 0.1 and 273.15 go up as they are
    # (clip_tabular cannot tell: clipping to the wide bound and then narrowing is clipping to the narrowed bound, rounding being monotone)
    assert {"mask_tabular", "mask_outside_range", "remove_extreme_values"} <= {c["filter"] for c in CASES if c["id"] in found}, found
    # and the statement that widens the column first is not the reference's either
    case = next(c for c in CASES if c["id"] == "seeded_300_00_mask_tabular")
    _, widened = R.statement(case["filter"], case["config"], case_table(case), round_scalars=False)
    assert not R.same_bits(widened["b"], R.expected_frame(GOLDEN, case)["b"])


def test_humidity_masked_by_the_masked_dewpoint_is_caught():
    hits = 0
    for case in CASES:
        if case["filter"] == "mask_dewpoint_temperature" and case["config"].get("mask_specific_humidity"):
            table = case_table(case)
            q = case["config"].get("specific_humidity", "2q")
            _, wrong = R.statement(case["filter"], case["config"], table, q_by_masked_td=True)
            assert not R.same_bits(wrong[q], R.expected_frame(GOLDEN, case)[q]), case["id"]
            assert not agree(interpreted(case["filter"], case["config"], table), ("columns", wrong)), case["id"]
            hits += 1
    assert hits >= 3
