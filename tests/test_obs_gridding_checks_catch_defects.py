"""The checks of tests/obs_gridding_checks.py, run on the CPU against a numpy stand-in of ``native.obs_best_per_cell`` and
``native.obs_fill_stack`` that walks the buffers as the kernels of csrc/atx_obs.hip do (pass 1: a minimum of uint64 score patterns per
slot; pass 2: a minimum of rows among equal patterns; the FIELDS fill by lanes of VEC points per target with the ``grid.y`` stride;
the COLUMNS fill by vectors of VEC levels) — once as it is (every check passes) and once per planted defect (the named case fails).
No deliberately broken kernel ever runs on a device.  The same file holds the checks' own reference: the loop against the recorded
grids of tests/golden/irregular_to_grid.json, against tests/obs_gridding_restatement.py and against its numpy broadcast."""

from __future__ import annotations

import struct

import numpy as np
import pytest
import torch

import obs_gridding_checks as C
import obs_gridding_restatement as R
from anemoi_transform_amd import obs

CPU = torch.device("cpu")
K = C.K
SMALL = C.Constants(block=K.block, wave=K.wave, grid_y=5)  # the grid.y cap of the stand-in: a handful of targets go past it
NAT = C.NAT
OUTSIDE = 777.0  # what a read outside the test's allocations gives the stand-in: a finite value


def pattern(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def wrap32(c: int) -> int:
    return (c + 2**31) % 2**32 - 2**31


class Memory:
    """The allocation a tensor lies in, as the kernel addresses it: flat from the tensor's first element, neighbours included."""

    def __init__(self, t: torch.Tensor, as_dtype=None):
        n = t.untyped_storage().nbytes() // t.element_size()
        self.flat = torch.as_strided(t, (n,), (1,), 0).numpy()
        if as_dtype is not None:
            self.flat = self.flat.view(as_dtype)
        self.base = t.storage_offset()

    def peek(self, i: int, outside):
        i += self.base
        return self.flat[i].item() if 0 <= i < len(self.flat) else outside

    def poke(self, i: int, v) -> None:
        i += self.base
        if 0 <= i < len(self.flat):
            self.flat[i] = v


# ---- the stand-in ---------------------------------------------------------------------------------------------------------------
class StandIn:
    def __init__(self, defect: str | None = None, k: C.Constants = SMALL):
        self.defect, self.k = defect, k
        self.routes = set()

    def kernels(self) -> C.Kernels:
        return C.Kernels(best_per_cell=self.best_per_cell, fill_stack=self.fill_stack)

    @staticmethod
    def pitch_of(values) -> int:
        n_cols, n_obs = values.shape
        return values.stride(0) if n_cols > 1 else max(n_obs, 1)

    # ---- obs_best_kernel<1>, obs_best_kernel<2> -------------------------------------------------------------------------------
    def score(self, diff: int, freq_ns: int, w: float, nan_count: int, n_cols: int) -> float:
        freq = float(freq_ns)
        share_of = n_cols - nan_count if self.defect == "the NaN share counts the columns that are not NaN" else nan_count
        if self.defect == "the NaN share by reciprocal multiplication":
            nan_score = float(share_of) * (1.0 / float(n_cols))
        else:
            nan_score = float(share_of) / float(n_cols)
        time_score = float(diff) * (1.0 / freq) if self.defect == "the time score by reciprocal multiplication" else float(diff) / freq
        if not w > 0.0:
            return time_score
        if self.defect == "the score contracted to one fma":
            return C.fma(1.0 - w, time_score, w * nan_score)
        a = (1.0 - w) * time_score
        b = w * nan_score
        return a + b

    def lane(self, r: int, date, cell, values, val_pitch, n_cols, targets, n_cells, win):
        """The (target, score pattern) pairs of row r, in the order the kernel's loop meets them."""
        defect = self.defect
        before, after, closed_before, closed_after, freq, w = win
        c = cell.peek(r, 0)
        if defect == "the cell narrowed to 32 bits before the range check":
            c = wrap32(c)
        if c < 0 or (c > n_cells if defect == "cell == n_cells accepted" else c >= n_cells):
            return None, []
        d = date.peek(r, 0)
        if d == NAT and defect != "a NaT row takes part":
            return None, []
        nan_count = 0
        for j in range(n_cols):
            v = values.peek(j * val_pitch + r, OUTSIDE)
            nan_count += 1 if v != v else 0
        if nan_count == n_cols and defect != "an all-NaN row takes part":
            return None, []
        if nan_count > 0 and defect == "a partly-NaN row dropped":
            return None, []
        out = []
        for t, tt in enumerate(targets):
            if tt == NAT and defect != "a NaT target not skipped":
                continue
            lo, hi = tt + before, tt + after
            if defect == "the two window ends swapped":
                lo, hi = hi, lo
            cb = closed_before != (defect == "the closure of the lower end inverted")
            ca = closed_after != (defect == "the closure of the upper end inverted")
            if not (d >= lo if cb else d > lo) or not (d <= hi if ca else d < hi):
                if defect == "an out-of-window target ends the row's loop":
                    break
                continue
            diff = d - tt
            if diff < 0 and defect != "abs of the difference missing":
                diff = -diff
            out.append((t, pattern(self.score(diff, freq, w, nan_count, n_cols))))
        return c, out

    def best_per_cell(self, date_ns, cell, values, target_ns, best, winner, *, n_cells, before_ns, after_ns, closed_before, closed_after, freq_ns, weight):
        n_cols, n_obs = values.shape
        n_time = target_ns.numel()
        val_pitch = self.pitch_of(values)
        if not (n_obs >= 0 and n_time >= 0 and n_cells >= 0 and n_cols > 0) or n_obs >= 2**31 or not freq_ns > 0 or not (0.0 <= weight <= 1.0):
            raise ValueError("atx_obs_best_per_cell: refused")
        assert val_pitch >= n_obs, "atx_obs_best_per_cell: val_pitch below n_obs"
        slots = n_time * n_cells
        if slots == 0:
            return
        best.fill_(-1)
        winner.fill_(-1)
        if n_obs == 0:
            return
        if self.defect == "values read at pitch n_obs by the score kernels":
            val_pitch = n_obs
        date, cells, vals = Memory(date_ns), Memory(cell), Memory(values)
        targets = target_ns.numpy().tolist()
        scores, rows = Memory(best, np.uint64), Memory(winner, np.uint32)
        win = (before_ns, after_ns, bool(closed_before), bool(closed_after), freq_ns, weight)
        n_rows = n_obs // self.k.block * self.k.block if self.defect == "the tail past the last full block dropped" else n_obs
        lanes = [self.lane(r, date, cells, vals, val_pitch, n_cols, targets, n_cells, win) for r in range(n_rows)]
        for r, (c, found) in enumerate(lanes):  # pass 1
            for t, bits in found:
                slot = t * n_cells + c
                if bits < scores.peek(slot, 0):
                    scores.poke(slot, bits)
        for r, (c, found) in enumerate(lanes):  # pass 2
            for t, bits in found:
                slot = t * n_cells + c
                if bits == scores.peek(slot, 0):
                    now = rows.peek(slot, 0)
                    if self.defect == "ties go to the higher row":
                        rows.poke(slot, r if now == 0xFFFFFFFF else max(now, r))
                    else:
                        rows.poke(slot, min(now, r))

    # ---- obs_fill_fields_kernel, obs_fill_columns_kernel ----------------------------------------------------------------------
    def value(self, winner: Memory, values: Memory, n_obs, val_pitch, n_cells, t, c, p) -> int:
        w = winner.peek(t * n_cells + p, 0)
        return self.value_of(w, values, n_obs, val_pitch, c)

    def value_of(self, w: int, values: Memory, n_obs, val_pitch, c) -> int:
        if w == -1 and self.defect == "an empty cell written as 0.0":
            return 0
        if w >= 0 and (w < n_obs or self.defect == "a winner >= n_obs dereferenced"):
            return values.peek(c * val_pitch + w, pattern(OUTSIDE))
        return C.QNAN

    def fill_stack(self, winner, values, out, *, n_time, n_cells, pitch, layout):
        defect, block = self.defect, self.k.block
        n_cols, n_obs = values.shape
        val_pitch = self.pitch_of(values)
        if not (n_obs >= 0 and n_time >= 0 and n_cells >= 0 and n_cols > 0) or n_obs >= 2**31 or layout not in (C.FIELDS, C.COLUMNS):
            raise ValueError("atx_obs_fill_stack: refused")
        assert val_pitch >= n_obs, "atx_obs_fill_stack: val_pitch below n_obs"
        n_lev = n_time * n_cols
        if n_lev == 0 or n_cells == 0:
            return
        assert pitch >= (n_lev if layout == C.COLUMNS else n_cells), "atx_obs_fill_stack: pitch too small"
        if defect == "values read at pitch n_obs by the fill":
            val_pitch = n_obs
        win, vals, stack = Memory(winner), Memory(values, np.uint64), Memory(out, np.uint64)
        vec = 2 if pitch % 2 == 0 and out.data_ptr() % 16 == 0 else 1
        self.routes.add(("FIELDS" if layout == C.FIELDS else "COLUMNS", vec))
        unwritten = defect == "the padding left unwritten"
        if layout == C.FIELDS:
            bx = (-(-pitch // vec) + block - 1) // block
            grid_y = min(n_time, self.k.grid_y)
            for item in range(bx * block):
                p0 = item * vec
                if p0 >= pitch:
                    continue
                for y in range(grid_y):
                    for t in range(y, n_time, grid_y):
                        if t != y and defect == "targets past the grid.y cap not filled":
                            break
                        w = [win.peek(t * n_cells + p0 + e, 0) if p0 + e < n_cells else None for e in range(vec)]
                        if defect == "the pair's second element takes the first's winner" and vec == 2 and w[1] is not None:
                            w[1] = w[0]
                        if defect == "a winner of -2 written as a padding zero":
                            w = [None if x == -2 else x for x in w]
                        for c in range(n_cols):
                            level = c * n_time + t if defect == "the level index as c * n_time + t" else t * n_cols + c
                            for e in range(vec):
                                if w[e] is None:
                                    if not (unwritten and p0 + e >= n_cells):
                                        stack.poke(level * pitch + p0 + e, 0)
                                else:
                                    stack.poke(level * pitch + p0 + e, self.value_of(w[e], vals, n_obs, val_pitch, c))
        else:
            vpr = pitch // vec
            for i in range(n_cells * vpr):
                p = i // vpr
                l0 = (i - p * vpr) * vec
                for e in range(vec):
                    level = l0 + e
                    if level < n_lev:
                        t, c = (level % n_cols, level // n_cols) if defect == "l / n_cols and l % n_cols swapped" else (level // n_cols, level % n_cols)
                        stack.poke(i * vec + e, self.value(win, vals, n_obs, val_pitch, n_cells, t, c, p))
                    elif not unwritten:
                        stack.poke(i * vec + e, 0)


# ---- the runs -------------------------------------------------------------------------------------------------------------------
def run_best(kern, rows=True, rounding=True, weights=True, windows=True, big=True, absent=True, targets=True, pitched=True, stray=True, refusals=True):
    if rows:
        for n in C.row_counts():
            C.check_best_row_count(kern, CPU, n)
    if rounding:
        for n_cols in C.ROUNDING_COLUMNS:
            C.check_best_rounding(kern, CPU, n_cols)
    if weights:
        for name in C.weight_tables():
            C.check_best_weight(kern, CPU, name)
    if windows:
        for name in C.window_tables():
            if windows is True or windows in name:
                C.check_best_window(kern, CPU, name)
    if big:
        C.check_best_big_difference(kern, CPU)
    if absent:
        for name in C.absent_tables():
            C.check_best_absent(kern, CPU, name)
    if targets:
        for name in C.target_tables():
            C.check_best_targets(kern, CPU, name)
    if pitched:
        for name in C.pitched_tables():
            C.check_best_pitched(kern, CPU, name)
    if stray:
        C.check_best_stray_cells(kern, CPU)
    if refusals:
        for name in C.refusal_calls():
            C.check_best_refusal(kern, CPU, name)


def only_best(**which):
    flags = dict(rows=False, rounding=False, weights=False, windows=False, big=False, absent=False, targets=False, pitched=False, stray=False, refusals=False)
    flags.update(which)
    return lambda kern: run_best(kern, **flags)


LAYOUTS = (C.FIELDS, C.COLUMNS)


def run_fill(kern, layouts=True, levels=True, many=True, end_to_end=True, stray=True, patterns=True, nothing=True):
    if layouts:
        for layout in LAYOUTS:
            for n_cells in C.fill_cell_counts():
                C.check_fill_layout(kern, CPU, layout, n_cells)
    if levels:
        for n_time, n_cols in C.COLUMN_SHAPES:
            C.check_fill_columns_levels(kern, CPU, n_time, n_cols)
    if many:
        for n_time in C.fill_target_counts(SMALL):
            C.check_fill_many_targets(kern, CPU, n_time)
    if end_to_end:
        C.check_end_to_end_many_targets(kern, CPU, SMALL)
    if stray:
        for layout in LAYOUTS:
            C.check_fill_stray_winners(kern, CPU, layout)
    if patterns:
        for layout in LAYOUTS:
            C.check_fill_bit_patterns(kern, CPU, layout)
    if nothing:
        for layout in LAYOUTS:
            C.check_fill_nothing(kern, CPU, layout)


def only_fill(**which):
    flags = dict(layouts=False, levels=False, many=False, end_to_end=False, stray=False, patterns=False, nothing=False)
    flags.update(which)
    return lambda kern: run_fill(kern, **flags)


def test_the_stand_in_passes_every_check_and_every_route_is_taken():
    stand_in = StandIn()
    kern = stand_in.kernels()
    run_best(kern)
    run_fill(kern)
    assert stand_in.routes == {("FIELDS", 1), ("FIELDS", 2), ("COLUMNS", 1), ("COLUMNS", 2)}


# defect -> (what to run, the assertion of the named case that catches it)
DEFECTS = {
    # the scores
    "the score contracted to one fma": (only_best(rounding=True), r"best per cell: rounding: pairs of equal real scores in both row orders, 3 columns: .*winners differ from the loop"),
    "the time score by reciprocal multiplication": (only_best(rounding=True), r"best per cell: rounding: pairs of equal real scores in both row orders, 3 columns: .*winners differ from the loop"),
    "the NaN share by reciprocal multiplication": (only_best(rounding=True), r"best per cell: rounding: pairs of equal real scores in both row orders, 5 columns: .*winners differ from the loop"),
    "the NaN share counts the columns that are not NaN": (only_best(weights=True), r"best per cell: w = 1.0: fewer NaNs win whatever the time: .*winners differ"),
    "ties go to the higher row": (only_best(weights=True), r"best per cell: w = 1.0: equal NaN counts, the first row wins whatever the time: .*winners differ"),
    "abs of the difference missing": (only_best(windows="window ends"), r"best per cell: window ends: .*winners differ from the loop, first \(target, cell\) \[\[0, 8\]\]"),
    # the window
    "the closure of the lower end inverted": (only_best(windows="window ends"), r"best per cell: window ends: closed_before = False, closed_after = False: .*first \(target, cell\) \[\[0, 1\]\]"),
    "the closure of the upper end inverted": (only_best(windows="window ends"), r"best per cell: window ends: closed_before = False, closed_after = False: .*first \(target, cell\) \[\[0, 4\]\]"),
    "the two window ends swapped": (only_best(windows="before > after"), r"best per cell: window: before > after: .*winners differ"),
    "an out-of-window target ends the row's loop": (only_best(windows="window ends"), r"best per cell: window ends: .*first \(target, cell\) \[\[2, 7\]\]"),
    # who takes part
    "a NaT row takes part": (only_best(absent=True), r"best per cell: rows that never take part: alone: .*first \(target, cell\) \[\[0, 0\]\]"),
    "a NaT target not skipped": (only_best(targets=True), r"best per cell: targets: a NaT target among good ones: .*first \(target, cell\) \[\[1, 0\]"),
    "an all-NaN row takes part": (only_best(absent=True), r"best per cell: rows that never take part: alone: .*first \(target, cell\) \[\[0, 1\]\]"),
    "a partly-NaN row dropped": (only_best(absent=True), r"best per cell: rows that never take part: alone: .*first \(target, cell\) \[\[0, 2\], \[0, 3\]\]"),
    "cell == n_cells accepted": (only_best(stray=True), r"best per cell: stray cells next to other targets' slots: .*written outside the winner or the score table"),
    "the cell narrowed to 32 bits before the range check": (only_best(stray=True), r"best per cell: stray cells next to other targets' slots: .*first \(target, cell\) \[\[0, 1\]"),
    # the walk
    "values read at pitch n_obs by the score kernels": (only_best(pitched=True), r"best per cell: pitched values: val_pitch = n_obs \+ 3, three columns: .*winners differ"),
    "the tail past the last full block dropped": (only_best(rows=True), r"best per cell: row counts: 1 rows: .*winners differ"),
    # the fill
    "a winner of -2 written as a padding zero": (only_fill(stray=True), r"fill: stray winners at real points: FIELDS, .*points without a winner hold no NaN.*kernel \[0\.0"),
    "the padding left unwritten": (only_fill(layouts=True), r"fill: layouts and pitches: FIELDS, .*padding elements are not zero bytes"),
    "an empty cell written as 0.0": (only_fill(layouts=True), r"fill: layouts and pitches: .*points without a winner hold no NaN"),
    "a winner >= n_obs dereferenced": (only_fill(stray=True), r"fill: stray winners at real points: .*points without a winner hold no NaN"),
    "targets past the grid.y cap not filled": (only_fill(many=True), r"fill: targets around the grid.y cap: FIELDS, n_time = 6, .*differ"),
    "the pair's second element takes the first's winner": (only_fill(layouts=True), r"fill: layouts and pitches: FIELDS, .* n_cells = 2, pitch = 2, base 0 bytes.*(differ|hold no NaN)"),
    "the level index as c * n_time + t": (only_fill(layouts=True), r"fill: layouts and pitches: FIELDS, .*(differ|hold no NaN)"),
    "l / n_cols and l % n_cols swapped": (only_fill(levels=True), r"fill: levels of the COLUMNS layout: COLUMNS, .*(differ|hold no NaN)"),
    "values read at pitch n_obs by the fill": (only_fill(patterns=True), r"fill: value bit patterns: .*val_pitch = \d+: .*differ in bits"),
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_named_case_catches_its_defect(defect):
    run, message = DEFECTS[defect]
    with pytest.raises(AssertionError, match=message) as caught:
        run(StandIn(defect=defect).kernels())
    print(f"{defect}: {str(caught.value)[:300]}")


def test_the_end_to_end_case_catches_the_cap_defect_too():
    with pytest.raises(AssertionError, match=r"fill: end to end past the grid.y cap: .*differ"):
        run_fill(StandIn(defect="targets past the grid.y cap not filled").kernels(), layouts=False, levels=False, many=False, stray=False, patterns=False, nothing=False)


# ---- the reference itself ---------------------------------------------------------------------------------------------------------
def small_tables() -> dict:
    out = {f"row counts: {n} rows": C.rows_table(n) for n in C.row_counts()}
    for n_cols in C.ROUNDING_COLUMNS:
        out[f"rounding, {n_cols} columns"] = C.rounding_table(n_cols)
    for tables in (C.weight_tables(), C.window_tables(), C.absent_tables(), C.target_tables(), C.pitched_tables()):
        out.update(tables)
    out["big differences"] = C.big_difference_table()
    out["stray cells"] = C.stray_cells_table()
    out["end to end, a small cap"] = C.end_to_end_table(SMALL)
    return out


SMALL_TABLES = small_tables()


@pytest.mark.parametrize("name", SMALL_TABLES)
def test_the_broadcast_and_the_restatement_equal_the_loop(name):
    tb = SMALL_TABLES[name]
    winner, best = C.winners_loop(tb)
    wide_winner, wide_best = C.winners_broadcast(tb)
    assert np.array_equal(wide_winner, winner) and np.array_equal(wide_best, best), f"{name}: the broadcast differs from the loop"
    if tb.expect is not None:
        assert winner.tolist() == tb.expect, f"{name}: the loop gives {winner.tolist()}"
    with np.errstate(over="ignore"):
        stack, restated = R.grid_observations(tb.date, tb.cell, tb.values, tb.targets, tb.n_cells, tb.window, tb.freq, tb.w)
    assert np.array_equal(restated, winner), f"{name}: the restatement differs from the loop"
    bits, real = C.fill_loop(winner, tb.values, C.FIELDS, tb.n_cells)
    assert bits.shape == stack.shape and np.array_equal(np.isnan(stack), np.isnan(bits.view(np.float64)))
    assert np.array_equal(C.u64(stack)[real], bits[real]), f"{name}: the restatement's fill differs from the fill loop"


@pytest.mark.parametrize("case", R.load_golden()["random_cases"], ids=lambda c: c["id"])
def test_the_loop_reproduces_the_recorded_reference_grids(case):
    config = case["config"]
    table = R.random_case_table(case)
    freq = obs.parse_frequency(config.get("time_freq", "6h"))
    window = tuple(obs.parse_window(config.get("window") or f"(-{config.get('time_freq', '6h')}, 0]"))
    targets = R.unique_in_order(table[config["window_date_column"]].astype("datetime64[ns]").view(np.int64))
    values = np.stack([table[c] for c in config["columns"]])
    tb = C.Table(table["date"].astype("datetime64[ns]").view(np.int64), table["spatial_index"], values, targets, case["n_cells"], window, freq=freq,
                 w=float(config.get("nan_score_weight", 0.0)))
    winner, _ = C.winners_loop(tb)
    bits, real = C.fill_loop(winner, values, C.FIELDS, case["n_cells"])
    want = R.expected_levels(case, case["n_cells"])
    assert np.isfinite(want).sum() > 300
    # a winner's own value may be NaN (a partly-NaN row): NaN where the recorded grid has one, the recorded bits elsewhere
    got = bits.view(np.float64)
    assert np.array_equal(np.isnan(want), got != got), "if the loop disagrees with the recorded grids, the loop is wrong"
    assert np.array_equal(C.u64(want)[got == got], bits[got == got]), "if the loop disagrees with the recorded grids, the loop is wrong"
    assert np.array_equal(C.winners_broadcast(tb)[0], winner)


def test_pairs_of_equal_real_scores_that_another_rounding_orders_differently():
    """The counts behind the rounding cases: of the (m, k) pairs at w = 0.25 and 6 h, how many each other score orders differently from
    two products and a sum; and that each changes a winner of the case that is there for it."""
    for n_cols, names in C.ROUNDING_COLUMNS.items():
        pairs, differing = C.equal_score_pairs(n_cols)
        counts = {name: len(found) for name, found in differing.items()}
        print(f"{n_cols} columns, {len(pairs)} pairs: {counts}")
        assert all(counts[name] >= 12 for name in names), counts
        tb = C.rounding_table(n_cols)
        want = C.winners_loop(tb)[0]
        changed = {name: int((C.winners_loop(tb, C.OTHER_SCORES[name])[0] != want).sum()) for name in names}
        print(f"winners of the rounding case changed: {changed} of {want.size}")
        assert all(changed.values())
    assert len(C.equal_score_pairs(3)[0]) == 2 * (719 - 41 + 1)
    assert all(k * (1.0 / 3) == k / 3 for k in range(4)) and 3 * (1.0 / 5) != 3 / 5


def test_the_edge_sizes_come_from_the_kernels_constants():
    """What the device module runs, at today's constants."""
    assert (K.block, K.wave, K.grid_y) == (256, 64, 65535)
    assert C.row_counts() == [1, 63, 65, 255, 256, 257, 769]
    assert C.walk_positions(769) == [0, 255, 767, 768] and C.walk_positions(257) == [0, 255, 256] and C.walk_positions(63) == [0, 62]
    assert C.fill_cell_counts() == [1, 2, 3, 511, 512, 513]
    assert C.fill_target_counts() == [65534, 65535, 65536, 65537] and len(C.end_to_end_table().targets) == 65537
    assert {n_cols for _, n_cols in C.COLUMN_SHAPES} == {1, 2, 3, 5} and {(t * c) % 2 for t, c in C.COLUMN_SHAPES} == {0, 1}
    assert C.stray_winners(23) == [-1, -2, -(2**31), 23, 24, 2**31 - 1]
