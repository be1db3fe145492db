"""Child process of tests/test_gpu_box_statistics.py::test_validation_mode_refuses_a_table_that_points_outside_the_stack: started with
ATX_VALIDATE=1 (the variable is read once per process), it hands atx_regrid_csr_stat tables with entries outside the stack and expects
each refused with the exact count, nothing written.

Every bad index is exactly n_src, one past the end, and the source tensor has a spare row there; indices and data have spare entries
past nnz: a library that failed to refuse would read allocated memory and give a wrong value, not fault."""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
from anemoi_transform_amd import native_stat  # noqa: E402
from anemoi_transform_amd.stack import COLUMNS  # noqa: E402

SENTINEL = 7.0
N_SRC, N_LEV, PITCH = 50, 5, 8


def main() -> None:
    assert os.environ.get("ATX_VALIDATE") == "1"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(21)
    values = 280.0 + 30.0 * rng.standard_normal((N_SRC + 1, PITCH))  # NaN-free; row N_SRC is the spare one
    src = torch.from_numpy(values).to(dev)
    refused = 0
    spare = 8
    for n_tgt, k in ((7, 3), (300, 4)):  # 21 entries: under one wave; 1200: several waves and a partial last one, no multiple of 64 or 256
        n = n_tgt * k
        idx = rng.integers(0, N_SRC, n).astype(np.int32)
        indptr = (np.arange(n_tgt + 1) * k).astype(np.int32)
        data = torch.from_numpy(np.concatenate([rng.random(n), np.zeros(spare)])).to(dev)
        out = torch.full((n_tgt, PITCH), SENTINEL, dtype=torch.float64, device=dev)

        def untouched() -> bool:
            torch.cuda.synchronize()
            return bool((out == SENTINEL).all())

        def run(pointers, columns, statistic, weights=data):
            columns = np.concatenate([columns, np.zeros(spare, dtype=np.int32)])
            native_stat.regrid_csr_stat(src, out, torch.from_numpy(pointers).to(dev), torch.from_numpy(columns).to(dev), weights, n_src=N_SRC,
                                        n_tgt=n_tgt, nnz=n, n_lev=N_LEV, src_pitch=PITCH, out_pitch=PITCH, layout=COLUMNS, statistic=statistic,
                                        policy="all", min_valid=0.0)

        # a valid table runs: the maximum of each row, with and without weights
        want = values[idx.reshape(n_tgt, k), :N_LEV].max(axis=1)
        for weights in (data, None):
            run(indptr, idx, "maximum", weights)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy()[:, :N_LEV], want)
            out.fill_(SENTINEL)

        last, three = idx.copy(), idx.copy()
        last[n - 1] = N_SRC
        three[list((5, 64 + 7, n - 1) if n > 128 else (2, 9, 17))] = N_SRC  # three different waves where the table has them
        bad_pointers = indptr.copy()
        bad_pointers[3] = n + 1
        cases = ((indptr, last, "indices", 1, N_SRC, "maximum"), (indptr, three, "indices", 3, N_SRC, "mode"),
                 (bad_pointers, idx, "indptr", 1, n + 1, "variance"))
        for pointers, columns, what, count, hi, statistic in cases:
            try:
                run(pointers, columns, statistic)
            except ValueError as e:
                assert "ATX_VALIDATE" in str(e) and f"found {count} entries of {what} outside [0, {hi})" in str(e), e
                assert untouched(), "a refused launch wrote"
                refused += 1
    print("refused", refused)


if __name__ == "__main__":
    main()
