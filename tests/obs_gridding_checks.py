"""The checks that hold the observation gridding kernels (csrc/atx_obs.hip: ``atx_obs_best_per_cell``, ``atx_obs_fill_stack``) to an
exact loop — written once, as plain functions over the callables under test and a device.  tests/test_gpu_obs_gridding_edges.py runs
them on ``native.obs_best_per_cell`` / ``native.obs_fill_stack`` on an MI355X; tests/test_obs_gridding_checks_catch_defects.py runs
them on the CPU against a numpy stand-in, once as it is and once per planted defect.

Every comparison is equality: winners and the score table as integers, stack values as bit patterns (a level that has a winner holds
that row's 8 bytes, NaN payload and zero sign included; a point without a winner holds A NaN, whichever), padding as all-zero
bytes, canaries and inputs as bytes.  No tolerance appears.

The reference shares nothing with the package and nothing with tests/obs_gridding_restatement.py: ``winners_loop`` is a Python loop
over targets and rows that states the header comment of atx_obs.hip literally — Python ints for nanoseconds (NaT is INT64_MIN),
Python floats for ``float(abs(d - t)) / float(freq)`` and ``(1.0 - w) * ts + w * (k / n)`` (two products, one sum, IEEE division for
both quotients), a strict ``<`` in row order — and ``fill_loop`` copies 8-byte patterns.  ``winners_broadcast`` is the same statement
as a numpy broadcast for the one case with more targets than the loop can afford; the CPU file holds it equal to the loop on every
small case, and holds the loop to the recorded grids of tests/golden/irregular_to_grid.json.

Sizes come from ``kBlock``, ``kWave`` and the ``grid.y`` cap of ``atx_obs_fill_stack``, read from the sources at import time.

Out of scope: the ``int64_t`` index route of the COLUMNS fill needs ``n_cells * pitch / vec >= 2^32`` vectors — tens of gigabytes of
stack on a shared card; and overflow of ``target + before``, which is the host parser's business.
"""

from __future__ import annotations

import os
import re
from dataclasses import dataclass
from fractions import Fraction
from typing import Callable, Optional

import numpy as np
import torch

from anemoi_transform_amd import native
from knn_superob_checks import Guarded, to_dev

FIELDS, COLUMNS = native.FIELDS, native.COLUMNS
NAT = -(2**63)
INT64_MAX, INT32_MIN, INT32_MAX = 2**63 - 1, -(2**31), 2**31 - 1
MINUTE = 60 * 10**9
H = 60 * MINUTE
T0 = 1_700_000_040 * 10**9  # 2023-11-14T22:14:00, a whole minute
QNAN = 0x7FF8000000000000
NAN_PATTERNS = {"quiet": QNAN, "quiet with a payload": 0x7FF8000000BEEF01, "negative": 0xFFF8000000000000,
                "signalling": 0x7FF0000000000001, "negative signalling": 0xFFF4000000000123}
ALL_ONES64 = 2**64 - 1


# ---- the kernels' constants ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Constants:
    block: int   # kBlock
    wave: int    # kWave
    grid_y: int  # the cap of grid.y in atx_obs_fill_stack: targets beyond it are reached by ``t += gridDim.y``


def read_constants() -> Constants:
    csrc = os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc")

    def find(name, pattern):
        with open(os.path.join(csrc, name)) as f:
            m = re.search(pattern, f.read())
        assert m, f"{name}: {pattern} not found"
        return int(m.group(1))

    return Constants(block=find("atx_common.hpp", r"constexpr int kBlock = (\d+);"), wave=find("atx_common.hpp", r"constexpr int kWave = (\d+);"),
                     grid_y=find("atx_obs.hip", r"\(unsigned\)\(n_time < (\d+) \? n_time : \1\)"))


K = read_constants()


@dataclass
class Kernels:
    """The callables under test, with the signatures of ``native.obs_best_per_cell(date_ns, cell, values, target_ns, best, winner, *,
    n_cells, before_ns, after_ns, closed_before, closed_after, freq_ns, weight)`` and ``native.obs_fill_stack(winner, values, out, *,
    n_time, n_cells, pitch, layout)``."""

    best_per_cell: Callable
    fill_stack: Callable


def f64(patterns) -> np.ndarray:
    """float64 values from 64-bit patterns."""
    return np.array(patterns, dtype=np.uint64).view(np.float64)


def u64(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64)


# ================================================================================================================================
# the reference
# ================================================================================================================================
def fma(a: float, b: float, c: float) -> float:
    """round(a * b + c), one rounding (``float(Fraction)`` is correctly rounded)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def plain_score(diff_ns: int, freq_ns: int, w: float, k: int, n: int) -> float:
    """The header comment of atx_obs.hip: ``diff_ns`` is |date - target|, ``k`` of the row's ``n`` columns are NaN."""
    ts = float(diff_ns) / float(freq_ns)
    if w <= 0:
        return ts
    return (1.0 - w) * ts + w * (k / n)


# what the statement is NOT: each must change a winner of the rounding cases, or those cases prove nothing
def fma_score(diff_ns, freq_ns, w, k, n):
    ts = float(diff_ns) / float(freq_ns)
    return ts if w <= 0 else fma(1.0 - w, ts, w * (k / n))


def reciprocal_time_score(diff_ns, freq_ns, w, k, n):
    ts = float(diff_ns) * (1.0 / float(freq_ns))
    return ts if w <= 0 else (1.0 - w) * ts + w * (k / n)


def reciprocal_share_score(diff_ns, freq_ns, w, k, n):
    ts = float(diff_ns) / float(freq_ns)
    return ts if w <= 0 else (1.0 - w) * ts + w * (float(k) * (1.0 / float(n)))


# (the other contraction, fma(w, k / n, (1.0 - w) * ts), changes nothing at w = 0.25: a product with a power of two is exact)
OTHER_SCORES = {"one fma": fma_score, "reciprocal time score": reciprocal_time_score, "reciprocal NaN share": reciprocal_share_score}


@dataclass
class Table:
    """One call of ``atx_obs_best_per_cell``.  ``values`` is ``[n_cols, n_obs]``; ``window`` is ``(before_ns, after_ns, closed_before,
    closed_after)``; the device sees ``values`` with rows ``n_obs + val_slack`` apart and ``gap`` in the slack."""

    date: np.ndarray
    cell: np.ndarray
    values: np.ndarray
    targets: np.ndarray
    n_cells: int
    window: tuple
    freq: int = 6 * H
    w: float = 0.0
    val_slack: int = 0
    gap: float = 4.5
    expect: Optional[list] = None  # the winners the case states, where it states them

    def __post_init__(self):
        self.date, self.cell = np.asarray(self.date, dtype=np.int64), np.asarray(self.cell, dtype=np.int64)
        self.targets = np.asarray(self.targets, dtype=np.int64)
        self.values = np.ascontiguousarray(self.values, dtype=np.float64)
        assert self.values.ndim == 2 and self.values.shape[1] == len(self.date) == len(self.cell)


def winners_loop(tb: Table, score: Callable = plain_score):
    """``(winner int32 [n_time, n_cells], best uint64 [n_time, n_cells])``: per target and cell the first row of smallest score and
    that score's bit pattern; -1 and all ones where no row takes part."""
    before, after, closed_before, closed_after = tb.window
    n_cols, n_obs = tb.values.shape
    dates, cells, targets = tb.date.tolist(), tb.cell.tolist(), tb.targets.tolist()
    columns = tb.values.tolist()
    nan_count = [sum(1 for j in range(n_cols) if columns[j][r] != columns[j][r]) for r in range(n_obs)]
    winner = np.full((len(targets), tb.n_cells), -1, dtype=np.int32)
    best = np.full((len(targets), tb.n_cells), ALL_ONES64, dtype=np.uint64)
    for t, target in enumerate(targets):
        if target == NAT:
            continue
        lo, hi = target + before, target + after
        smallest = {}
        for r in range(n_obs):
            d, c, k = dates[r], cells[r], nan_count[r]
            if d == NAT or k == n_cols or not 0 <= c < tb.n_cells:
                continue
            if not (d >= lo if closed_before else d > lo):
                continue
            if not (d <= hi if closed_after else d < hi):
                continue
            s = score(abs(d - target), tb.freq, tb.w, k, n_cols)
            if c not in smallest or s < smallest[c][0]:
                smallest[c] = (s, r)
        for c, (s, r) in smallest.items():
            winner[t, c] = r
            best[t, c] = np.array([s]).view(np.uint64)[0]
    return winner, best


def winners_broadcast(tb: Table):
    """The same statement as one numpy broadcast over (target, row), for the case with more than ``grid_y`` targets."""
    before, after, closed_before, closed_after = tb.window
    n_cols, n_obs = tb.values.shape
    n_time = len(tb.targets)
    winner = np.full((n_time, tb.n_cells), -1, dtype=np.int32)
    best = np.full((n_time, tb.n_cells), ALL_ONES64, dtype=np.uint64)
    if n_obs == 0 or n_time == 0 or tb.n_cells == 0:
        return winner, best
    k = (tb.values != tb.values).sum(axis=0)
    row_ok = (tb.date != NAT) & (k < n_cols) & (tb.cell >= 0) & (tb.cell < tb.n_cells)
    d, t = tb.date[None, :], tb.targets[:, None]
    with np.errstate(over="ignore"):
        lo, hi = t + np.int64(before), t + np.int64(after)
        ok = ((d >= lo) if closed_before else (d > lo)) & ((d <= hi) if closed_after else (d < hi)) & row_ok[None, :] & (t != NAT)
        ts = np.abs(d - t).astype(np.float64) / np.float64(tb.freq)
    s = ts if tb.w <= 0 else (1.0 - tb.w) * ts + tb.w * (k / n_cols)[None, :]
    s = np.where(ok, s, np.inf)
    rows_at = np.arange(n_time)
    for c in np.unique(tb.cell[row_ok]).tolist():
        rows = np.flatnonzero(row_ok & (tb.cell == c))
        sub = s[:, rows]
        j = np.argmin(sub, axis=1)  # the first of equal minima: the lowest row
        m = sub[rows_at, j]
        found = np.isfinite(m)
        winner[found, c] = rows[j][found]
        best[found, c] = m[found].view(np.uint64)
    return winner, best


def fill_loop(winner: np.ndarray, values: np.ndarray, layout: int, pitch: int):
    """``(stack uint64 [n_lev or n_cells, pitch], real bool of the same shape)``: level ``t * n_cols + c`` of point ``p`` is the 8 bytes of
    ``values[c][winner[t][p]]`` (``real``) or a NaN where ``winner[t][p]`` is no row of the table; padding is zero bytes."""
    n_time, n_cells = winner.shape
    n_cols, n_obs = values.shape
    n_lev = n_time * n_cols
    shape = (n_lev, pitch) if layout == FIELDS else (n_cells, pitch)
    out, real = np.zeros(shape, dtype=np.uint64), np.zeros(shape, dtype=bool)
    patterns = [row.tolist() for row in u64(values).reshape(n_cols, n_obs)]
    rows = winner.tolist()
    for t in range(n_time):
        for p in range(n_cells):
            w = rows[t][p]
            for c in range(n_cols):
                level = t * n_cols + c
                at = (level, p) if layout == FIELDS else (p, level)
                if 0 <= w < n_obs:
                    out[at], real[at] = patterns[c][w], True
                else:
                    out[at] = QNAN
    return out, real


# ================================================================================================================================
# atx_obs_best_per_cell
# ================================================================================================================================
BEST_GARBAGE, BEST_CANARY = 1, 0x0123456789ABCDEF  # garbage below every score: a table not reset lets no row in
WINNER_GARBAGE, WINNER_CANARY = 0, -7777


def run_best(kern: Kernels, device, name: str, tb: Table, want=None):
    """Every input a view between canaries (dates and cells that WOULD win), the value rows ``n_obs + val_slack`` apart, ``best`` and
    ``winner`` pre-filled with garbage between canaries.  Every winner and every score pattern equals the loop's."""
    n_cols, n_obs = tb.values.shape
    n_time = len(tb.targets)
    pitch = n_obs + tb.val_slack
    vhost = np.full((n_cols, pitch), tb.gap)
    vhost[:, :n_obs] = tb.values
    vals = Guarded(vhost, device, tb.gap, guard=4)
    ontime = int(tb.targets[0]) if n_time and tb.targets[0] != NAT else T0
    dates = Guarded(tb.date, device, ontime, guard=4)
    cells = Guarded(tb.cell, device, 0, guard=4)
    tgts = Guarded(tb.targets, device, ontime, guard=4)
    best = Guarded(np.full((n_time, tb.n_cells), BEST_GARBAGE, np.int64), device, BEST_CANARY)
    winner = Guarded(np.full((n_time, tb.n_cells), WINNER_GARBAGE, np.int32), device, WINNER_CANARY)
    before, after, closed_before, closed_after = tb.window
    kern.best_per_cell(dates.view, cells.view, vals.view[:, :n_obs], tgts.view, best.view, winner.view, n_cells=tb.n_cells, before_ns=before,
                       after_ns=after, closed_before=closed_before, closed_after=closed_after, freq_ns=tb.freq, weight=tb.w)
    got_w = winner.view.cpu().numpy().reshape(n_time, tb.n_cells)
    got_b = best.view.cpu().numpy().reshape(n_time, tb.n_cells).view(np.uint64)
    want_w, want_b = winners_loop(tb) if want is None else want
    label = (f"best per cell: {name}: n_obs = {n_obs}, n_cols = {n_cols}, val_pitch = {pitch}, n_time = {n_time}, n_cells = {tb.n_cells}, "
             f"window = {tb.window}, freq = {tb.freq}, w = {tb.w!r}")
    assert winner.canaries_intact() and best.canaries_intact(), f"{label}: written outside the winner or the score table"
    if n_time * tb.n_cells and n_obs == 0:
        assert np.all(got_w == -1) and np.all(got_b == ALL_ONES64), f"{label}: an empty table leaves every winner -1 and every score all ones"
    bad = np.argwhere(got_w != want_w)
    assert bad.size == 0, (f"{label}: {len(bad)} winners differ from the loop, first (target, cell) {bad[:4].tolist()}: kernel {[int(got_w[t, c]) for t, c in bad[:4]]}, "
                           f"loop {[int(want_w[t, c]) for t, c in bad[:4]]}")
    bad = np.argwhere(got_b != want_b)
    assert bad.size == 0, (f"{label}: {len(bad)} score patterns differ from the loop, first (target, cell) {bad[:4].tolist()}: kernel {[hex(got_b[t, c]) for t, c in bad[:4]]}, "
                           f"loop {[hex(want_b[t, c]) for t, c in bad[:4]]}")
    if tb.expect is not None:
        assert want_w.tolist() == tb.expect, f"{label}: the loop gives {want_w.tolist()}, the case states {tb.expect}"
    assert vals.unchanged() and dates.unchanged() and cells.unchanged() and tgts.unchanged(), f"{label}: an input was modified"
    return got_w


def complete(n_cols: int, n_obs: int) -> np.ndarray:
    """Values without a NaN that name their (row, column)."""
    return np.arange(n_obs, dtype=np.float64)[None, :] * 16.0 + np.arange(n_cols, dtype=np.float64)[:, None] + 0.5


# ---- row counts -----------------------------------------------------------------------------------------------------------------
def row_counts(k: Constants = K) -> list:
    return [1, k.wave - 1, k.wave + 1, k.block - 1, k.block, k.block + 1, 3 * k.block + 1]


def walk_positions(n: int, k: Constants = K) -> list:
    """First and last lane of the first and of the last block, and the last lane of the last whole block."""
    last = (n - 1) // k.block * k.block
    return sorted({0, min(k.block, n) - 1, max(last - 1, 0), last, n - 1})


def rows_table(n: int, k: Constants = K) -> Table:
    """Five targets a day apart.  Cell 0: target j has its one row of score 0 at the j-th walk position.  Cells 1 .. 3: dates on a
    10-minute lattice on both sides of the targets, so that rows of different blocks have equal scores; cell 3 holds no row of the first
    block.  Two columns with NaNs, w = 0.25."""
    rng = np.random.default_rng(n)
    targets = T0 + np.arange(5, dtype=np.int64) * 24 * H
    date = targets[rng.integers(0, 5, n)] + rng.integers(1, 6, n) * rng.choice([-10, 10], n) * MINUTE
    cell = rng.integers(0, 4, n).astype(np.int64)
    cell[(cell == 3) & (np.arange(n) < k.block)] = 2
    values = complete(2, n)
    values[rng.random((2, n)) < 0.2] = np.nan
    for j, r in enumerate(walk_positions(n, k)):
        date[r], cell[r], values[:, r] = targets[j], 0, (r, -r)
    return Table(date, cell, values, targets, 5, (-3 * H, 3 * H, True, True), w=0.25)


def ties_across_blocks(tb: Table, k: Constants = K) -> int:
    """The (target, cell) pairs whose smallest score is held by rows of different blocks."""
    winner, best = winners_loop(tb)
    n_cols = tb.values.shape[0]
    nan_count = (tb.values != tb.values).sum(axis=0)
    seen = 0
    for t, c in np.argwhere(winner >= 0).tolist():
        target = int(tb.targets[t])
        blocks = set()
        for r in np.flatnonzero(tb.cell == c).tolist():
            d = int(tb.date[r])
            if nan_count[r] < n_cols and target - 3 * H <= d <= target + 3 * H:
                s = plain_score(abs(d - target), tb.freq, tb.w, int(nan_count[r]), n_cols)
                if np.array([s]).view(np.uint64)[0] == best[t, c]:
                    blocks.add(r // k.block)
        seen += len(blocks) > 1
    return seen


def check_best_row_count(kern: Kernels, device, n: int, k: Constants = K) -> None:
    tb = rows_table(n, k)
    want = winners_loop(tb)
    for j, r in enumerate(walk_positions(n, k)):
        assert want[0][j, 0] == r and want[1][j, 0] == 0, "the walked row wins cell 0 of its target with score +0.0"
    if n >= 2 * k.block:
        assert ties_across_blocks(tb, k) >= 2, "rows of different blocks hold the smallest score of a cell"
        assert np.any(want[0][:, 3] >= k.block), "a cell whose rows all lie past the first block"
    run_best(kern, device, f"row counts: {n} rows", tb, want=want)


# ---- the score's rounding -------------------------------------------------------------------------------------------------------
def sign(a: float, b: float) -> int:
    return (a > b) - (a < b)


ROUNDING_COLUMNS = {3: ("one fma", "reciprocal time score"), 5: ("one fma", "reciprocal time score", "reciprocal NaN share")}


def equal_score_pairs(n_cols: int = 3, w: float = 0.25, freq: int = 6 * H):
    """Row A ``m`` minutes from the target with ``k`` NaNs, row B ``m - 120 / n_cols`` minutes with ``k + 1``: equal scores as real
    numbers at w = 0.25 and 6 h (40 minutes for three columns, 24 for five).  ``(pairs, differing)``: all (m, k) for m up to 719 and
    k + 1 < n_cols, and per other score the pairs it orders differently.  With three columns ``k * (1.0 / 3)`` IS ``k / 3`` for k = 1
    and 2, so no table of three columns can tell a reciprocal NaN share; ``3 * (1.0 / 5)`` is not ``3 / 5``: hence the five."""
    gap = 120 // n_cols
    assert gap * n_cols == 120
    pairs, differing = [], {name: [] for name in OTHER_SCORES}
    for m in range(gap + 1, 720):
        for k in range(n_cols - 2) if n_cols > 3 else (0, 1):
            a, b = (m * MINUTE, k), ((m - gap) * MINUTE, k + 1)
            exact = [Fraction(1.0 - w) * Fraction(d, freq) + Fraction(w) * Fraction(kk, n_cols) for d, kk in (a, b)]
            assert exact[0] == exact[1]
            pairs.append((m, k))
            base = sign(plain_score(a[0], freq, w, a[1], n_cols), plain_score(b[0], freq, w, b[1], n_cols))
            for name, other in OTHER_SCORES.items():
                if sign(other(a[0], freq, w, a[1], n_cols), other(b[0], freq, w, b[1], n_cols)) != base:
                    differing[name].append((m, k))
    return pairs, differing


def pairs_table(pairs, w: float, n_cols: int = 3, freq: int = 6 * H) -> Table:
    """Each pair in two cells of its own: A before B, and B before A.  All rows before the one target, window (-12 h, 0]."""
    gap = 120 // n_cols
    date, cell, nans = [], [], []
    for i, (m, k) in enumerate(pairs):
        a, b = (T0 - m * MINUTE, k), (T0 - (m - gap) * MINUTE, k + 1)
        for c, order in ((2 * i, (a, b)), (2 * i + 1, (b, a))):
            for d, kk in order:
                date.append(d)
                cell.append(c)
                nans.append(kk)
    values = complete(n_cols, len(date))
    for r, kk in enumerate(nans):
        values[:kk, r] = np.nan
    return Table(date, cell, values, [T0], 2 * len(pairs), (-12 * H, 0, False, True), freq=freq, w=w)


def rounding_table(n_cols: int = 3) -> Table:
    """w = 0.25, 6 h: up to 12 pairs per other score, chosen where that score orders the pair differently."""
    _, differing = equal_score_pairs(n_cols)
    chosen = []
    for name in ROUNDING_COLUMNS[n_cols]:
        found = differing[name]
        assert found, f"no pair of equal scores is ordered differently by: {name}"
        chosen += [p for p in found[:: max(1, len(found) // 12)][:12] if p not in chosen]
    return pairs_table(chosen, 0.25, n_cols)


def check_best_rounding(kern: Kernels, device, n_cols: int) -> None:
    tb = rounding_table(n_cols)
    want = winners_loop(tb)
    assert np.all(want[0] >= 0)
    for name in ROUNDING_COLUMNS[n_cols]:
        changed = int((winners_loop(tb, OTHER_SCORES[name])[0] != want[0]).sum())
        assert changed > 0, f"the rounding case does not tell the statement from: {name}"
    run_best(kern, device, f"rounding: pairs of equal real scores in both row orders, {n_cols} columns", tb, want=want)


def weight_tables() -> dict:
    """name -> Table for w = 1.0, the smallest positive w and w = 0, each with pairs in both row orders."""
    tiny = 5e-324
    out = {}
    # w = 1: the score is k / n alone.  (m, k) against (m - 40, k + 1): A wins in both orders; equal k: the first row wins
    tb = pairs_table([(100, 0), (500, 1), (41, 0)], 1.0)
    tb.expect = [[0, 3, 4, 7, 8, 11]]
    out["w = 1.0: fewer NaNs win whatever the time"] = tb
    date = [T0 - 30 * MINUTE, T0 - 500 * MINUTE, T0 - 500 * MINUTE, T0 - 30 * MINUTE]
    values = complete(3, 4)
    values[0, :] = np.nan
    out["w = 1.0: equal NaN counts, the first row wins whatever the time"] = Table(date, [0, 0, 1, 1], values, [T0], 2, (-12 * H, 0, False, True), w=1.0, expect=[[0, 2]])
    # the smallest positive w: 1.0 - w is 1.0, w * (1 / 3) rounds to +0.0 and w * (2 / 3) to w: only at time score 0 does it show
    assert 1.0 - tiny == 1.0 and tiny * (1 / 3) == 0.0 and tiny * (2 / 3) == tiny
    date = [T0, T0, T0, T0, T0, T0, T0 - MINUTE, T0 - 2 * MINUTE, T0 - 2 * MINUTE, T0 - MINUTE]
    cell = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    nans = [2, 0, 1, 0, 0, 2, 2, 0, 0, 2]
    values = complete(3, 10)
    for r, kk in enumerate(nans):
        values[:kk, r] = np.nan
    out["the smallest positive w"] = Table(date, cell, values, [T0], 5, (-12 * H, 0, False, True), w=tiny, expect=[[1, 2, 4, 6, 9]])
    # w = 0: NaN counts must not matter
    date = [T0 - 10 * MINUTE, T0 - 10 * MINUTE, T0 - 20 * MINUTE, T0 - 10 * MINUTE, T0 - 10 * MINUTE, T0 - 10 * MINUTE]
    cell = [0, 0, 1, 1, 2, 2]
    nans = [2, 0, 0, 2, 0, 1]
    values = complete(3, 6)
    for r, kk in enumerate(nans):
        values[:kk, r] = np.nan
    out["w = 0: NaN counts do not matter"] = Table(date, cell, values, [T0], 3, (-12 * H, 0, False, True), w=0.0, expect=[[0, 3, 4]])
    return out


def check_best_weight(kern: Kernels, device, name: str) -> None:
    run_best(kern, device, name, weight_tables()[name])


# ---- window ends ----------------------------------------------------------------------------------------------------------------
CLOSURES = ((False, False), (False, True), (True, False), (True, True))


def window_tables() -> dict:
    out = {}
    before, after = -6 * H, 3 * H
    targets = [T0, T0 + 24 * H, T0 + 48 * H]
    for closed_before, closed_after in CLOSURES:
        lo, hi = T0 + before, T0 + after
        # cells 0 .. 5: one row each, a nanosecond either side of and on each end; cell 6: the nearer row is LATER than the target;
        # cell 7: a row inside the window of target 2 only; cell 8: the nearer row is EARLIER than the target and the farther one later
        date = [lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, T0 - 2 * H, T0 + 1 * H, T0 + 48 * H - 1 * H, T0 + 2 * H, T0 - 1 * H]
        cell = [0, 1, 2, 3, 4, 5, 6, 6, 7, 8, 8]
        first = [-1, 1 if closed_before else -1, 2, 3, 4 if closed_after else -1, -1, 7, -1, 10]
        expect = [first, [-1] * 9, [-1] * 7 + [8, -1]]
        out[f"window ends: closed_before = {closed_before}, closed_after = {closed_after}"] = Table(
            date, cell, complete(2, 11), targets, 9, (before, after, closed_before, closed_after), w=0.25, expect=expect)
        # before == after: the one instant belongs to the window only when both ends are closed
        at = T0 - 1 * H
        out[f"window: before == after, closed_before = {closed_before}, closed_after = {closed_after}"] = Table(
            [at - 1, at, at + 1], [0, 1, 2], complete(1, 3), [T0], 3, (-1 * H, -1 * H, closed_before, closed_after),
            expect=[[-1, 1 if closed_before and closed_after else -1, -1]])
    # before > after: no instant lies in the window, though the rows lie between the two ends
    out["window: before > after"] = Table([T0 - 1 * H, T0, T0 + 1 * H, T0 - 1], [0, 1, 2, 1], complete(1, 4), [T0], 3, (1 * H, -1 * H, True, True), expect=[[-1, -1, -1]])
    return out


def check_best_window(kern: Kernels, device, name: str) -> None:
    run_best(kern, device, name, window_tables()[name])


def big_difference_table() -> Table:
    """|date - target| of 2^53, 2^53 + 1, 2^53 + 2 ns at freq = 1 ns, on both sides of the target: the first two convert to the same
    double and tie (the lower row wins although it is the farther one), the third is strictly larger."""
    e = 2**53
    assert float(e + 1) == float(e) and float(e + 2) == e + 2.0 > float(e)
    date = [T0 - (e + 1), T0 - e, T0 - (e + 2), T0 - (e + 1), T0 + e + 1, T0 + e, T0 + e + 2, T0 - e, T0 + e + 2, T0 - (e + 2)]
    cell = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    return Table(date, cell, complete(1, 10), [T0], 5, (-(2**54), 2**54, False, False), freq=1, expect=[[0, 3, 4, 7, 8]])


def check_best_big_difference(kern: Kernels, device) -> None:
    run_best(kern, device, "differences of 2^53, 2^53 + 1 and 2^53 + 2 ns", big_difference_table())


# ---- rows and targets that take no part -----------------------------------------------------------------------------------------
def absent_tables() -> dict:
    """One target at -1000 ns with the closed window [INT64_MIN, target]: a NaT row lies INSIDE it by its number alone."""
    n_cells, target = 6, -1000
    window = (NAT - target, 0, True, True)
    nan = NAN_PATTERNS
    #         NaT     all-NaN rows (two columns)                            cells outside the grid
    date = [NAT] + [target - 5] * 3 + [target - 5] * 5
    cell = [0, 1, 1, 1, -1, n_cells, 2**32 + 1, NAT, INT64_MAX]
    values = complete(2, 9)
    values[:, 1] = f64([nan["quiet"], nan["quiet with a payload"]])
    values[:, 2] = f64([nan["negative"], nan["negative signalling"]])
    values[:, 3] = f64([nan["signalling"], nan["negative"]])
    # a partly-NaN row takes part (cell 2), one with a signalling NaN as well (cell 3)
    partly = complete(2, 2) + 1000.0
    partly[0, 0] = np.nan
    partly[1, 1] = f64([nan["signalling"]])[0]
    alone = Table(date + [target - 7, target - 9], cell + [2, 3], np.hstack([values, partly]), [target], n_cells, window, w=0.5,
                  expect=[[-1, -1, 9, 10, -1, -1]])
    good = complete(2, 6) + 5000.0
    beside = Table(date + [target - 7, target - 9] + [target - 100] * 6, cell + [2, 3] + list(range(6)), np.hstack([values, partly, good]), [target], n_cells, window,
                   w=0.5, expect=[[11, 12, 13, 14, 15, 16]])
    return {"rows that never take part: alone": alone, "rows that never take part: next to good rows": beside}


def target_tables() -> dict:
    out = {}
    # a NaT target among good ones; rows just above INT64_MIN lie in (NaT + 0, NaT + 1 h] by their numbers alone
    date = [NAT + 1, NAT + 1000, NAT + 1 * H, T0 + 30 * MINUTE, T0 + 6 * H + 1]
    out["targets: a NaT target among good ones"] = Table(date, [0, 1, 2, 0, 1], complete(2, 5), [T0, NAT, T0 + 6 * H], 3, (0, 1 * H, False, True), w=0.25,
                                                        expect=[[3, -1, -1], [-1, -1, -1], [-1, 4, -1]])
    rng = np.random.default_rng(12)
    n = 60
    targets = np.array([T0 + 12 * H, T0, T0 + 6 * H, T0 + 12 * H, T0], dtype=np.int64)
    values = complete(2, n)
    values[rng.random((2, n)) < 0.3] = np.nan
    out["targets: duplicated and unsorted"] = Table(T0 + rng.integers(-6 * 60, 12 * 60, n) * MINUTE, rng.integers(0, 4, n), values, targets, 4,
                                                   (-6 * H, 0, False, True), w=0.25)
    one = Table([T0 - MINUTE], [0], complete(1, 1), [T0], 1, (-6 * H, 0, False, True))
    out["n_time = 0"] = Table(one.date, one.cell, one.values, [], 3, one.window)
    out["n_cells = 0"] = Table(one.date, one.cell, one.values, [T0, T0 + H], 0, one.window)
    out["n_obs = 0"] = Table([], [], np.zeros((2, 0)), [T0, T0 + H, NAT], 4, one.window, w=0.5, expect=[[-1] * 4] * 3)
    return out


def check_best_absent(kern: Kernels, device, name: str) -> None:
    run_best(kern, device, name, absent_tables()[name])


def check_best_targets(kern: Kernels, device, name: str) -> None:
    tb = target_tables()[name]
    got = run_best(kern, device, name, tb)
    if name == "targets: duplicated and unsorted":
        assert np.array_equal(got[0], got[3]) and np.array_equal(got[1], got[4]) and np.any(got[0] != got[1]) and np.all((got >= 0).sum(axis=1) >= 3)


# ---- pitched values, stray cells --------------------------------------------------------------------------------------------------
def pitched_tables() -> dict:
    """Value rows ``n_obs + 3`` apart with finite values in the gap.  In every cell the nearer row has a NaN in columns 1 and 2 and the
    farther one none; w = 0.9 makes the NaN count decide.  Read at pitch ``n_obs``, column 1 and 2 of a row are other rows' values or
    the gap and the counts change."""
    n_cells = 24
    n = 2 * n_cells
    date = np.where(np.arange(n) % 2 == 0, T0 - 10 * MINUTE, T0 - 50 * MINUTE)
    cell = np.arange(n) // 2
    values = complete(3, n)
    values[1:, 0::2] = np.nan
    values[0, 1::4] = np.nan
    three = Table(date, cell, values, [T0], n_cells, (-6 * H, 0, False, True), w=0.9, val_slack=3, gap=-3.25)
    one = Table(date, cell, values[:1].copy(), [T0], n_cells, (-6 * H, 0, False, True), w=0.9, val_slack=3, gap=-3.25)
    return {"pitched values: val_pitch = n_obs + 3, three columns": three, "pitched values: one column": one}


def read_at_pitch_n_obs(tb: Table) -> Table:
    """What a kernel that ignores ``val_pitch`` sees."""
    n_cols, n_obs = tb.values.shape
    flat = np.full((n_cols, n_obs + tb.val_slack), tb.gap)
    flat[:, :n_obs] = tb.values
    return Table(tb.date, tb.cell, flat.reshape(-1)[: n_cols * n_obs].reshape(n_cols, n_obs), tb.targets, tb.n_cells, tb.window, tb.freq, tb.w)


def check_best_pitched(kern: Kernels, device, name: str) -> None:
    tb = pitched_tables()[name]
    if tb.values.shape[0] > 1:
        assert np.any(winners_loop(read_at_pitch_n_obs(tb))[0] != winners_loop(tb)[0]), "values read at pitch n_obs change a winner"
    run_best(kern, device, name, tb)


def stray_cells_table() -> Table:
    """Three targets, four cells, every slot won by a row half an hour off.  Rows ON each target with cells -1, n_cells and
    2^32 + 1: taken as addresses they would be the neighbouring target's last or first cell, cell 1, or the canaries."""
    targets = [T0, T0 + 24 * H, T0 + 48 * H]
    date, cell = [], []
    for t in targets:
        date += [t - 30 * MINUTE] * 4 + [t] * 3
        cell += [0, 1, 2, 3, -1, 4, 2**32 + 1]
    return Table(date, cell, complete(2, len(date)), targets, 4, (-6 * H, 0, False, True), w=0.25,
                 expect=[[0, 1, 2, 3], [7, 8, 9, 10], [14, 15, 16, 17]])


def check_best_stray_cells(kern: Kernels, device) -> None:
    run_best(kern, device, "stray cells next to other targets' slots", stray_cells_table())


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def refusal_calls() -> dict:
    """name -> the changes to a good call that the entry point must refuse before it launches or resets anything."""
    return {"n_cols = 0": {"n_cols": 0}, "freq = 0": {"freq_ns": 0}, "freq < 0": {"freq_ns": -6 * H}, "w < 0": {"weight": -0.25}, "w > 1": {"weight": 1.5},
            "w NaN": {"weight": float("nan")}, "val_pitch < n_obs": {"val_pitch": 7}}


def check_best_refusal(kern: Kernels, device, name: str) -> None:
    change = refusal_calls()[name]
    n_obs, n_cols = 8, change.get("n_cols", 2)
    store = to_dev(complete(1, 4 * n_obs).reshape(-1), device)
    values = torch.as_strided(store, (n_cols, n_obs), (change.get("val_pitch", n_obs), 1))
    dates, cells, tgts = to_dev(np.full(n_obs, T0 - MINUTE), device), to_dev(np.zeros(n_obs, np.int64), device), to_dev(np.array([T0]), device)
    best = Guarded(np.full((1, 3), BEST_GARBAGE, np.int64), device, BEST_CANARY)
    winner = Guarded(np.full((1, 3), WINNER_GARBAGE, np.int32), device, WINNER_CANARY)
    label = f"best per cell: refusals: {name}"
    good = torch.as_strided(store, (2, n_obs), (n_obs, 1))
    kern.best_per_cell(dates, cells, good, tgts, best.view.clone(), accepted := winner.view.clone(), n_cells=3, before_ns=-6 * H, after_ns=0, closed_before=False,
                       closed_after=True, freq_ns=6 * H, weight=0.25)
    assert accepted.cpu().numpy().tolist() == [[0, -1, -1]], f"{label}: the call without the change is a good one"
    try:
        kern.best_per_cell(dates, cells, values, tgts, best.view, winner.view, n_cells=3, before_ns=-6 * H, after_ns=0, closed_before=False, closed_after=True,
                           freq_ns=change.get("freq_ns", 6 * H), weight=change.get("weight", 0.25))
    except (ValueError, AssertionError) as e:  # ATX_EINVAL, ATX_ESHAPE as native raises them
        refusal = e
    else:
        refusal = None
    assert refusal is not None, f"{label}: the call was accepted"
    assert best.unchanged() and winner.unchanged(), f"{label}: a refused call wrote to its tables"


# ================================================================================================================================
# atx_obs_fill_stack
# ================================================================================================================================
OUT_GARBAGE, OUT_CANARY = -6.02e23, 8.25e11
OUT_GUARD = 16


def named_values(n_cols: int, n_obs: int) -> np.ndarray:
    """``1000 * column + row``: a value names the (row, column) it was read from."""
    return np.arange(n_cols, dtype=np.float64)[:, None] * 1000.0 + np.arange(n_obs, dtype=np.float64)[None, :]


def random_winners(rng, n_time: int, n_cells: int, n_obs: int) -> np.ndarray:
    """A handmade table: a different row at every point and target where there is one, -1 at about a quarter."""
    w = rng.integers(0, max(n_obs, 1), (n_time, n_cells)).astype(np.int32)
    w[rng.random((n_time, n_cells)) < 0.25] = -1
    if n_obs == 0:
        w[:] = -1
    return w


def run_fill(kern: Kernels, device, name: str, winner: np.ndarray, values: np.ndarray, layout: int, pitch: int, val_slack: int = 0, gap: float = 4.5,
             off16: int = 0, want=None) -> None:
    """The stack ``off16`` bytes past a 16-byte boundary inside an allocation of garbage between canaries, ``winner`` between canaries
    that name row 0, the value rows ``n_obs + val_slack`` apart.  Levels equal ``fill_loop``, padding is zero bytes, nothing else
    changes."""
    winner = np.ascontiguousarray(winner, dtype=np.int32)
    n_time, n_cells = winner.shape
    n_cols, n_obs = values.shape
    n_lev = n_time * n_cols
    rows, used = (n_lev, n_cells) if layout == FIELDS else (n_cells, n_lev)
    size = rows * pitch
    host = np.full(size + 2 * OUT_GUARD + 2, OUT_GARBAGE)
    backing = torch.from_numpy(host.copy()).to(device)
    start = OUT_GUARD + ((off16 - backing.data_ptr() - 8 * OUT_GUARD) % 16) // 8
    host[:start], host[start + size:] = OUT_CANARY, OUT_CANARY
    backing.copy_(torch.from_numpy(host))
    out = torch.as_strided(backing, (rows, pitch), (pitch, 1), start)
    assert out.data_ptr() % 16 == off16
    vhost = np.full((n_cols, n_obs + val_slack), gap)
    vhost[:, :n_obs] = values
    vals = Guarded(vhost, device, gap, guard=4)
    win = Guarded(winner, device, 0, guard=4)
    kern.fill_stack(win.view, vals.view[:, :n_obs], out, n_time=n_time, n_cells=n_cells, pitch=pitch, layout=layout)
    got = backing.cpu().numpy().view(np.uint64)
    label = (f"fill: {name}: {'FIELDS' if layout == FIELDS else 'COLUMNS'}, n_time = {n_time}, n_cols = {n_cols}, n_cells = {n_cells}, pitch = {pitch}, "
             f"base {off16} bytes past a 16-byte boundary, n_obs = {n_obs}, val_pitch = {n_obs + val_slack}")
    before = host.view(np.uint64)
    assert np.array_equal(got[:start], before[:start]) and np.array_equal(got[start + size:], before[start + size:]), f"{label}: written outside the stack"
    assert win.unchanged() and vals.unchanged(), f"{label}: an input was modified"
    if n_lev == 0 or n_cells == 0:
        assert np.array_equal(got, before), f"{label}: a stack of nothing was written to"
        return
    stack = got[start: start + size].reshape(rows, pitch)
    want_bits, real = fill_loop(winner, values, layout, pitch) if want is None else want
    levels, want_levels, real = stack[:, :used], want_bits[:, :used], real[:, :used]
    bad = np.argwhere(real & (levels != want_levels))
    assert bad.size == 0, (f"{label}: {len(bad)} values differ in bits from the winner's, first at {bad[:4].tolist()}: kernel {[hex(levels[i, j]) for i, j in bad[:4]]}, "
                           f"loop {[hex(want_levels[i, j]) for i, j in bad[:4]]}")
    isnan = levels.view(np.float64) != levels.view(np.float64)
    bad = np.argwhere(~real & ~isnan)
    assert bad.size == 0, (f"{label}: {len(bad)} points without a winner hold no NaN, first at {bad[:4].tolist()}: kernel {[float(levels.view(np.float64)[i, j]) for i, j in bad[:4]]}, "
                           f"winners {sorted(set(winner.reshape(-1)[(winner.reshape(-1) < 0) | (winner.reshape(-1) >= n_obs)].tolist()))[:8]}")
    bad = np.argwhere(stack[:, used:] != 0)
    assert bad.size == 0, f"{label}: {len(bad)} padding elements are not zero bytes, first at {bad[:4].tolist()}: {[hex(stack[i, used + j]) for i, j in bad[:4]]}"


def fill_cell_counts(k: Constants = K) -> list:
    return [1, 2, 3, 2 * k.block - 1, 2 * k.block, 2 * k.block + 1]


def check_fill_layout(kern: Kernels, device, layout: int, n_cells: int) -> None:
    """Two targets, two columns; pitches from tight to three spare elements (odd: VEC = 1; even and tight; even and larger: the
    second element of the last vector is padding), each from an aligned base and from one 8 bytes off (VEC = 1 again)."""
    n_time, n_cols, n_obs = 2, 2, 37
    used = n_cells if layout == FIELDS else n_time * n_cols
    values = named_values(n_cols, n_obs)
    for spare in range(4):
        for off16 in (0, 8):
            winner = random_winners(np.random.default_rng(10 * n_cells + spare), n_time, n_cells, n_obs)
            run_fill(kern, device, "layouts and pitches", winner, values, layout, used + spare, off16=off16)


COLUMN_SHAPES = ((1, 1), (1, 2), (2, 1), (3, 1), (2, 2), (1, 3), (2, 3), (3, 3), (1, 5), (2, 5), (3, 5))  # (n_time, n_cols)


def check_fill_columns_levels(kern: Kernels, device, n_time: int, n_cols: int) -> None:
    """COLUMNS: level ``t * n_cols + c`` of every point names (winner[t][p], c).  ``pitch = n_lev`` and larger; with an odd ``n_cols``
    and an even pitch a 16-byte vector holds the last column of one target and the first of the next."""
    n_lev, n_obs, n_cells = n_time * n_cols, 41, 67
    values = named_values(n_cols, n_obs)
    for spare in range(3):
        winner = random_winners(np.random.default_rng(100 * n_lev + spare), n_time, n_cells, n_obs)
        if n_time > 1:
            assert np.any(winner[0] != winner[1])
        run_fill(kern, device, "levels of the COLUMNS layout", winner, values, COLUMNS, n_lev + spare)


def fill_target_counts(k: Constants = K) -> list:
    return [k.grid_y - 1, k.grid_y, k.grid_y + 1, k.grid_y + 2]


def check_fill_many_targets(kern: Kernels, device, n_time: int) -> None:
    """FIELDS over 3 cells and one column with a target count around the cap of ``grid.y``: pitch 4 (VEC = 2) and 3 (VEC = 1)."""
    n_obs = 29
    rng = np.random.default_rng(n_time)
    winner = random_winners(rng, n_time, 3, n_obs)
    winner[-1] = [5, -1, 28]
    values = named_values(1, n_obs)
    for pitch in (4, 3):
        run_fill(kern, device, "targets around the grid.y cap", winner, values, FIELDS, pitch)


def end_to_end_table(k: Constants = K) -> Table:
    """``grid_y + 2`` targets a minute apart over 3 cells, a few hundred rows with NaNs."""
    n_time, n = k.grid_y + 2, 200
    rng = np.random.default_rng(k.grid_y)
    targets = T0 + np.arange(n_time, dtype=np.int64) * MINUTE
    date = T0 + rng.integers(0, n_time * 6, n) * (MINUTE // 6)
    date[:3] = targets[-1]  # the last target's own rows
    values = complete(2, n)
    values[rng.random((2, n)) < 0.3] = np.nan
    values[:, :3] = complete(2, 3)
    return Table(date, rng.permutation(n) % 3, values, targets, 3, (-20 * H, 10 * H, False, True), w=0.25)


def check_end_to_end_many_targets(kern: Kernels, device, k: Constants = K) -> None:
    """Both kernels, one after the other, past the cap; the winners by the broadcast, the stack by the fill loop."""
    tb = end_to_end_table(k)
    want = winners_broadcast(tb)
    assert (want[0] >= 0).mean() > 0.5 and len(np.unique(want[0])) > min(100, len(tb.targets) // 2)
    winner = run_best(kern, device, "end to end past the grid.y cap", tb, want=want)
    run_fill(kern, device, "end to end past the grid.y cap", winner, tb.values, FIELDS, 4)


def stray_winners(n_obs: int) -> list:
    return [-1, -2, INT32_MIN, n_obs, n_obs + 1, INT32_MAX]


def check_fill_stray_winners(kern: Kernels, device, layout: int) -> None:
    """Every stray winner at real points — first, last and inner ones, in either element of a pair — between good ones: a NaN in both
    layouts, never an address (the two value rows past ``n_obs`` are finite slack of the test's own)."""
    n_obs, n_time, n_cols, n_cells = 23, 2, 2, 11
    values = named_values(n_cols, n_obs)
    winner = np.arange(n_time * n_cells, dtype=np.int32).reshape(n_time, n_cells) % n_obs
    for j, w in enumerate(stray_winners(n_obs)):
        winner[0, j], winner[1, n_cells - 1 - j] = w, w
    used = n_cells if layout == FIELDS else n_time * n_cols
    for pitch in (used, used + 1, used + 2, used + 3):
        run_fill(kern, device, "stray winners at real points", winner, values, layout, pitch, val_slack=2, gap=-3.25)


def special_values() -> np.ndarray:
    """Two columns of patterns that a copy keeps and arithmetic may not."""
    patterns = list(NAN_PATTERNS.values()) + [0x8000000000000000, 0x0000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001,
                                              0x800FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0x3FF0000000000000, 0xBFF0000000000001]
    return np.stack([f64(patterns), f64(patterns[::-1])])


def check_fill_bit_patterns(kern: Kernels, device, layout: int) -> None:
    """NaN payloads (signalling ones too), -0.0, ±inf and subnormals arrive bit for bit; the value rows are pitched."""
    values = special_values()
    n_cols, n_obs = values.shape
    n_time, n_cells = 2, n_obs + 3
    winner = (np.arange(n_time * n_cells, dtype=np.int32).reshape(n_time, n_cells) * 7) % n_obs
    winner[1, 2] = -1
    assert set(winner.reshape(-1).tolist()) >= set(range(n_obs))
    used = n_cells if layout == FIELDS else n_time * n_cols
    for pitch in (used + used % 2, used + 1 - used % 2):  # even (VEC = 2) and odd
        run_fill(kern, device, "value bit patterns", winner, values, layout, pitch, val_slack=3, gap=-3.25)


def check_fill_nothing(kern: Kernels, device, layout: int) -> None:
    """``n_obs = 0`` with an all -1 table: NaN everywhere; no levels, no points: nothing is written."""
    for pitch in (6, 7):
        run_fill(kern, device, "an empty table", np.full((2, 3) if layout == COLUMNS else (2, 5), -1, np.int32), np.zeros((3, 0)), layout, pitch)
    run_fill(kern, device, "no levels", np.zeros((0, 5), np.int32), named_values(2, 4), layout, 6)
    run_fill(kern, device, "no points", np.zeros((3, 0), np.int32), named_values(2, 4), layout, 6)
