"""`bench.py --dump-outputs` on the host: which target points are written, and how the output stack (whole, or the shards of
N ranks) becomes DIR/regrid_out.npy.  No GPU: the stacks live in host memory."""

from __future__ import annotations

import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_dump_targets_fill_the_budget_with_a_fixed_sample(bench):
    assert np.array_equal(bench.dump_targets(65160, 7, 8), np.arange(65160))  # a stack that fits is written whole
    pick = bench.dump_targets(1038240, 137, 8)  # the headline's stack: 1.1 GB
    assert len(pick) * 137 * 8 <= bench.DUMP_BYTES < (len(pick) + 1) * 137 * 8 and bench.DUMP_BYTES <= 64 * 2**20
    assert np.all(np.diff(pick) > 0) and pick[0] >= 0 and pick[-1] < 1038240
    assert np.array_equal(pick, bench.dump_targets(1038240, 137, 8))  # seeded: the same points in every run
    assert len(bench.dump_targets(1038240, 137, 4)) == bench.DUMP_BYTES // (137 * 4)


def _stack(want, layout):
    from anemoi_transform_amd.stack import COLUMNS, Stack

    n_lev, n_pts = want.shape
    st = Stack.empty(n_pts, n_lev, torch.float64, torch.device("cpu"), layout, zero=True)
    if layout == COLUMNS:
        st.data[:, :n_lev] = torch.from_numpy(want.T)
    else:
        st.data[:, :] = torch.from_numpy(want)
    return st


@pytest.mark.parametrize("layout_name", ["columns", "fields"])
def test_dump_is_field_major_at_the_sampled_targets(bench, tmp_path, monkeypatch, layout_name):
    from anemoi_transform_amd.stack import COLUMNS, FIELDS

    n_lev, n_tgt = 5, 1000
    want = np.random.default_rng(1).standard_normal((n_lev, n_tgt))
    monkeypatch.setattr(bench, "DUMP_BYTES", 300 * n_lev * 8)  # room for 300 of the 1000 targets
    layout = COLUMNS if layout_name == "columns" else FIELDS
    bench.dump_outputs(str(tmp_path / "out"), _stack(want, layout), 0, n_tgt, n_tgt, 0, 1, None)
    got = np.load(tmp_path / "out" / "regrid_out.npy")
    pick = bench.dump_targets(n_tgt, n_lev, 8)
    assert len(pick) == 300 and got.dtype == np.float64 and np.array_equal(got, want[:, pick])


def test_dump_of_two_ranks_joins_their_target_ranges(bench, tmp_path, monkeypatch):
    """Rank r holds the targets [lo, hi) of its shard; rank 0 writes the sample of the whole grid, in target order."""
    from anemoi_transform_amd.stack import COLUMNS

    n_lev, n_tgt, cut = 3, 800, 333
    want = np.random.default_rng(2).standard_normal((n_lev, n_tgt))
    monkeypatch.setattr(bench, "DUMP_BYTES", 200 * n_lev * 8)
    sent = []

    class Rank1Group:
        def gather_object(self, obj, parts, dst):
            assert parts is None and dst == 0
            sent.append(obj)

    bench.dump_outputs(str(tmp_path / "rank1"), _stack(want[:, cut:], COLUMNS), cut, n_tgt, n_tgt, 1, 2, Rank1Group())
    assert not os.path.exists(tmp_path / "rank1") and len(sent) == 1  # only rank 0 writes

    class Rank0Group:
        def gather_object(self, obj, parts, dst):
            assert dst == 0
            parts[:] = [obj, sent[0]]

    bench.dump_outputs(str(tmp_path / "rank0"), _stack(want[:, :cut], COLUMNS), 0, cut, n_tgt, 0, 2, Rank0Group())
    pick = bench.dump_targets(n_tgt, n_lev, 8)
    assert np.array_equal(np.load(tmp_path / "rank0" / "regrid_out.npy"), want[:, pick])
