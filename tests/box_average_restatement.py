"""Grid-box-average weights in this project's own words: plain Python loops over target cells, source rows and source cells, with
one-at-a-time defects, and the checks that the host and the GPU tests share.

The statement (``interp.box_average_rows`` holds it in full): row ``r`` spans the latitude edges 90, the midpoints between row
latitudes, -90; ``z = sin(deg2rad(edge))`` with the poles set to +-1 exactly; source row ``q`` takes part in target row ``r`` iff
``dz = min(zt[r], zs[q]) - max(zt[r+1], zs[q+1]) > 2**-40 * (zt[r] - zt[r+1])``; cell ``j`` of ``n`` is the arc
``[(j - 1/2) 360/n, (j + 1/2) 360/n)`` on the circle, whose edges in units of ``360 / (2 ns nt)`` are integers, so the overlap ``ov``
is an exact integer; ``raw = dz * (ov / (2 ns nt))``; entries in ascending source index; ``tot`` summed from 0 in that order;
``w = raw / tot``.  ``defect=`` switches on ONE wrong variant, each a mistake a builder could make; ``run_checks`` catches each by the
check named for it in ``DEFECTS``.

Only for small grids: every target cell visits every source cell.
"""

from __future__ import annotations

import math

import numpy as np

from anemoi_transform_amd.grids import row_structure

# name -> (source grid, target grid)
PAIRS = {
    "O8->F4": ("O8", "F4"),
    "O8->30deg": ("O8", [30.0, 30.0]),
    "30deg->O8": ([30.0, 30.0], "O8"),  # upsampling: rows of 1-4 entries
    "10deg->30deg": ([10.0, 10.0], [30.0, 30.0]),
    "O16->O4": ("O16", "O4"),
    "O12->22.5deg": ("O12", [22.5, 22.5]),
    "7.2deg->36deg": ([7.2, 7.2], [36.0, 36.0]),  # aligned edges that differ in the last bit: the sliver rule
}
IDENTITIES = {"O8->O8": ("O8", "O8"), "15deg->15deg": ([15.0, 15.0], [15.0, 15.0])}

# defect -> the message of the check in run_checks that catches it
DEFECTS = {
    "cell0_no_wrap": "column sums",
    "edges_at_row_latitudes": "column sums",
    "z_is_latitude": "column sums",
    "pairwise_sum": "matrix_data differs",
    "no_sliver_rule": "every source cell once",
    "unsorted_wrap": "ascending",
}


def rows_of(grid):
    rows = row_structure(grid)
    assert rows is not None, grid
    return rows


def edges_z(rows, defect: str | None = None) -> list[float]:
    lats = [float(x) for x in rows[0]]
    edges = [90.0]
    for r in range(1, len(lats)):
        edges.append(lats[r] if defect == "edges_at_row_latitudes" else (lats[r - 1] + lats[r]) / 2)
    edges.append(-90.0)
    if defect == "z_is_latitude":
        return [e / 90.0 for e in edges]
    z = [float(np.sin(np.deg2rad(e))) for e in edges]
    z[0], z[-1] = 1.0, -1.0
    return z


def overlap(i: int, nt: int, j: int, ns: int, defect: str | None = None) -> int:
    """Length of the intersection of target cell i (of nt) and source cell j (of ns) in units of 360 / (2 ns nt) degrees."""
    units = 2 * ns * nt
    a0, len_a = (2 * i - 1) * ns, 2 * ns
    b0, len_b = (2 * j - 1) * nt, 2 * nt
    if defect == "cell0_no_wrap":  # intervals on a line: cell 0 reaches below 0 and meets nothing there
        return max(0, min(a0 + len_a, b0 + len_b) - max(a0, b0))
    d = (b0 - a0) % units  # the source arc is [d, d + len_b) where the target arc is [0, len_a)
    return max(0, min(len_a, d + len_b) - d) + max(0, min(len_a, d + len_b - units))


def pairwise(values: list[float]) -> float:
    if len(values) <= 2:
        return sum(values, 0.0)
    half = len(values) // 2
    return pairwise(values[:half]) + pairwise(values[half:])


def box_average(src_rows, tgt_rows, defect: str | None = None) -> dict[str, np.ndarray]:
    assert defect is None or defect in DEFECTS, defect
    zs, zt = edges_z(src_rows, defect), edges_z(tgt_rows, defect)
    slen, tlen = [int(n) for n in src_rows[1]], [int(n) for n in tgt_rows[1]]
    sstart = [sum(slen[:q]) for q in range(len(slen))]
    data, indices, indptr = [], [], [0]
    for r, nt in enumerate(tlen):
        for i in range(nt):
            entries = []
            for q, ns in enumerate(slen):
                dz = min(zt[r], zs[q]) - max(zt[r + 1], zs[q + 1])
                if not dz > (0.0 if defect == "no_sliver_rule" else 2.0**-40 * (zt[r] - zt[r + 1])):
                    continue
                cells = [(k + ns - ns // 2) % ns for k in range(ns)] if defect == "unsorted_wrap" else range(ns)
                for j in cells:
                    ov = overlap(i, nt, j, ns, defect)
                    if ov > 0:
                        entries.append((sstart[q] + j, dz * (float(ov) / float(2 * ns * nt))))
            if defect == "pairwise_sum":
                tot = pairwise([raw for _, raw in entries])
            else:
                tot = 0.0
                for _, raw in entries:
                    tot += raw
            for column, raw in entries:
                indices.append(column)
                data.append(raw / tot)
            indptr.append(len(indices))
    return dict(matrix_data=np.array(data, dtype=np.float64), matrix_indices=np.array(indices, dtype=np.int32),
                matrix_indptr=np.array(indptr, dtype=np.int32), matrix_shape=np.array([sum(tlen), sum(slen)]))


_STATEMENTS: dict[str, dict[str, np.ndarray]] = {}


def statement(name: str) -> dict[str, np.ndarray]:
    """The clean restatement of a pair of PAIRS or IDENTITIES, evaluated once per process; the arrays are read-only."""
    if name not in _STATEMENTS:
        src, tgt = {**PAIRS, **IDENTITIES}[name]
        _STATEMENTS[name] = box_average(rows_of(src), rows_of(tgt))
        for a in _STATEMENTS[name].values():
            a.flags.writeable = False
    return _STATEMENTS[name]


def cell_areas(rows) -> np.ndarray:
    """Area of every cell as a share of the sphere's: dz / 2 per row, split evenly among its cells (the true edges, no defect)."""
    z = edges_z(rows)
    return np.concatenate([np.full(int(n), (z[r] - z[r + 1]) / 2 / int(n)) for r, n in enumerate(rows[1])])


def check_equal(got: dict, want: dict, what: str) -> None:
    for key in ("matrix_indptr", "matrix_indices", "matrix_data"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), f"{what}: {key} differs"
    assert np.array_equal(got["matrix_shape"], want["matrix_shape"]), f"{what}: matrix_shape differs"


def check_invariants(matrix: dict, src_rows, tgt_rows, what: str) -> None:
    data, indices, indptr = matrix["matrix_data"], matrix["matrix_indices"].astype(np.int64), matrix["matrix_indptr"].astype(np.int64)
    n_tgt, n_src = (int(n) for n in matrix["matrix_shape"])
    assert (n_tgt, n_src) == (int(np.sum(tgt_rows[1])), int(np.sum(src_rows[1]))) and len(indptr) == n_tgt + 1, f"{what}: shape"
    assert indptr[0] == 0 and indptr[-1] == len(indices) == len(data) and np.all(np.diff(indptr) >= 1), f"{what}: indptr"
    assert indices.min() >= 0 and indices.max() < n_src, f"{what}: index range"
    assert np.all(data > 0), f"{what}: a weight is not positive"
    tgt_area, src_area = cell_areas(tgt_rows), cell_areas(src_rows)
    column_sums = np.zeros(n_src)
    constant = 287.5
    for t in range(n_tgt):
        lo, hi = indptr[t], indptr[t + 1]
        assert np.all(np.diff(indices[lo:hi]) > 0), f"{what}: indices of target {t} are not strictly ascending: {indices[lo:hi]}"
        total, field = 0.0, 0.0
        for p in range(lo, hi):
            total += float(data[p])
            field += float(data[p]) * constant
        assert abs(total - 1.0) <= (hi - lo + 1) * 2.0**-52, f"{what}: row sum of target {t} is off by {total - 1.0}"
        assert abs(field - constant) <= 1e-15 * constant, f"{what}: a constant field comes back off by {field - constant} at target {t}"
        column_sums[indices[lo:hi]] += tgt_area[t] * data[lo:hi]
    worst = np.max(np.abs(column_sums - src_area) / src_area)
    assert worst <= 1e-13, f"{what}: area-weighted column sums differ from the source cell areas by {worst} relative"


def check_identity(matrix: dict, what: str) -> None:
    n = int(matrix["matrix_shape"][0])
    assert np.array_equal(matrix["matrix_indices"], np.arange(n)) and np.array_equal(matrix["matrix_indptr"], np.arange(n + 1)), \
        f"{what}: identical grids do not give the identity pattern"
    assert np.all(matrix["matrix_data"] == 1.0), f"{what}: identical grids give weights other than 1.0"


def run_checks(builder, pairs=None) -> None:
    """Every check of the issue on ``builder(src_rows, tgt_rows) -> matrix``: the invariants on every pair, the identities, the sliver
    pair, and last the bits against the clean restatement."""
    names = list(PAIRS) + list(IDENTITIES) if pairs is None else list(pairs)
    built = {}
    for name in names:
        src, tgt = ({**PAIRS, **IDENTITIES})[name]
        built[name] = builder(rows_of(src), rows_of(tgt))
        check_invariants(built[name], rows_of(src), rows_of(tgt), name)
    for name in names:
        if name in IDENTITIES:
            check_identity(built[name], name)
    if "7.2deg->36deg" in built:
        m = built["7.2deg->36deg"]
        assert len(m["matrix_indices"]) == 1300 == int(m["matrix_shape"][1]) and \
            np.array_equal(np.sort(m["matrix_indices"]), np.arange(1300)), \
            f"7.2deg->36deg: every source cell once: {len(m['matrix_indices'])} entries for 1300 source cells"
    for name in names:
        check_equal(built[name], statement(name), name)


assert math.isclose(float(np.sum(cell_areas(rows_of("O8")))), 1.0, rel_tol=1e-14)
