"""The tile plan of the three column-tile kernels (``atx_levels_interpolate``, ``atx_geopotential_on_model_levels``,
``atx_heights_interpolate``; csrc/atx_column_tile.hpp) restated in plain Python: how a stack is staged (``column_route``), the LDS a tile
of ``pt`` points takes in each kernel (``levels_carve``, ``geo_carve``, ``heights_carve``), the points of a tile (``tile_points``) and the
variables the heights kernel stages at a time (``heights_chunk``) — and ``TILE_CASES``, the shapes the GPU test
(tests/test_gpu_column_tile.py) runs because of what the tile does at them.  It shares no code with the package: the four constants are
read from the header's text, everything else is written out again here, so that the host test (tests/test_column_tile_host.py) can hold
it to the library's own refusal message, which prints the LDS of one point.

A stack's storage is ``(aligned, pitch)``: whether its base is 16-byte aligned, and the elements between two points' columns.  The
storage strings are those of ``hybrid_column_common.allocate``.
"""

from __future__ import annotations

import os
import re
from typing import NamedTuple, Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "anemoi-transform_amd", "csrc", "atx_column_tile.hpp")


def constant(name: str) -> int:
    """``constexpr <type> name = <products of integers>;`` of the header."""
    (found,) = re.findall(r"constexpr \w+ " + name + r" = ([0-9* ]+);", open(HEADER).read())
    value = 1
    for factor in found.split("*"):
        value *= int(factor)
    return value


BLOCK = constant("kTileBlock")
MAX_POINTS = constant("kTileMaxPoints")
LDS_PREFERRED = constant("kTileLdsPreferred")
LDS_LIMIT = constant("kTileLdsLimit")

COLUMN_STORAGE = ("columns", "columns-pitch+1", "columns-base+1")
LEVELS, GEOPOTENTIAL, HEIGHTS = "levels", "geopotential", "heights"
WHOLE, GROUND, SEA = "whole", "ground", "sea"  # the spellings of geopotential_restatement and heights_restatement


class Plan(NamedTuple):
    PT: int                  # points of a tile; 0: refused
    budget: Optional[int]    # LDS_PREFERRED or LDS_LIMIT; None: refused
    lds_bytes: int           # the dynamic LDS of the launch; of a refused call: what one point needs, as the message prints it
    tiles: int
    chunk: Optional[int]     # heights: the variables staged at a time

    @property
    def refused(self) -> bool:
        return self.PT == 0

    def last_tile(self, n_pts: int) -> int:
        """The points of the last tile."""
        return n_pts - (self.tiles - 1) * self.PT


# ---- csrc/atx_column_tile.hpp ------------------------------------------------------------------------------------------------------
def round16(n: int) -> int:
    return (n + 15) // 16 * 16


def vec(T) -> int:
    """Elements of a 16-byte vector."""
    return 16 // np.dtype(T).itemsize


def column_route(aligned: bool, pitch: int, rows: int, V: int) -> tuple[bool, int]:
    """``(vector, lds_pitch)``: 16 bytes per lane iff the base is aligned, the pitch a whole number of vectors and the vectors that
    cover the rows end inside the pitch; lds_pitch is then the covered elements, the rows themselves otherwise."""
    covered = (rows + V - 1) // V * V
    vector = aligned and pitch % V == 0 and covered <= pitch
    return vector, covered if vector else rows


def tile_points(one_tile) -> tuple[int, Optional[int]]:
    """``(PT, budget)``: the largest pt <= MAX_POINTS whose ``one_tile(pt)`` bytes fit LDS_PREFERRED — found by halving steps, as the
    header does — or, if not even one point fits, the same under LDS_LIMIT; ``(0, None)`` if one point does not fit that either."""
    for budget in (LDS_PREFERRED, LDS_LIMIT):
        pt, step = 0, MAX_POINTS
        while step > 0:
            if pt + step <= MAX_POINTS and one_tile(pt + step) <= budget:
                pt += step
            step //= 2
        if pt > 0:
            return pt, budget
    return 0, None


def storage_form(storage: str, rows: int, T) -> tuple[bool, int]:
    """``(aligned, pitch)`` of a ``[n_pts, rows]`` view that ``hybrid_column_common.allocate`` makes for the storage string."""
    per16 = vec(T)
    pitch = -(-max(rows, 1) // per16) * per16
    if storage == "columns-pitch+1":
        pitch += 1
    assert storage in COLUMN_STORAGE, storage
    return storage != "columns-base+1", pitch


def plan_of(one_tile, n_pts: int, chunk_of=None) -> Plan:
    PT, budget = tile_points(one_tile)
    if PT == 0:
        return Plan(0, None, one_tile(1), 0, None)
    return Plan(PT, budget, one_tile(PT), (n_pts + PT - 1) // PT, None if chunk_of is None else chunk_of(PT))


# ---- csrc/levels/atx_levels.hip ------------------------------------------------------------------------------------------------------
def levels_carve(pt: int, lds_pitch: int, elem: int, n_lev: int, n_tgt: int) -> int:
    """The bytes of a tile of pt points: the staged columns, p_full, sp, p_ground, the brackets' w, a and b, the monotone flags, and
    the four coefficients of every row."""
    total = round16(pt * lds_pitch * elem)       # T [pt][lds_pitch]
    total += round16(pt * n_lev * 8)             # double [pt][n_lev]
    total += round16(pt * 8)                     # double [pt]
    total += round16(pt * 8)                     # double [pt]
    total += round16(pt * n_tgt * 8)             # double [pt][n_tgt]
    total += round16(pt * n_tgt * 4)             # int [pt][n_tgt]
    total += round16(pt * n_tgt * 4)             # int [pt][n_tgt]
    total += round16(pt * 4)                     # int [pt]
    total += round16(4 * n_lev * 8)              # double [4][n_lev]
    return total


def levels_plan_of(T, n_pts: int, n_lev: int, n_tgt: int, n_var: int, src: tuple[bool, int]) -> Plan:
    elem = np.dtype(T).itemsize
    _, lds_pitch = column_route(*src, n_var * n_lev, vec(T))
    return plan_of(lambda pt: levels_carve(pt, lds_pitch, elem, n_lev, n_tgt), n_pts)


def levels_plan(T, shape, storage: str = "columns") -> Plan:
    """``shape``: (n_pts, n_lev, n_tgt, n_var), as ``levels_restatement.SHAPES``."""
    n_pts, n_lev, n_tgt, n_var = shape
    return levels_plan_of(T, n_pts, n_lev, n_tgt, n_var, storage_form(storage, n_var * n_lev, T))


# ---- csrc/geopotential/atx_geopotential.hip ------------------------------------------------------------------------------------------
def geo_carve(pt: int, lt: int, lq: int, elem: int, n_lev: int) -> int:
    """The staged t and q columns — a float64 stack's terms take their places, a float32 stack's two float64 arrays of an odd pitch —
    sp, zs and the two coefficients of the n_lev + 1 half levels."""
    total = round16(pt * lt * elem) + round16(pt * lq * elem)
    if elem != 8:
        odd = n_lev | 1
        total += round16(pt * odd * 8) + round16(pt * odd * 8)
    total += round16(pt * 8) + round16(pt * 8)
    total += round16(2 * (n_lev + 1) * 8)
    return total


def geo_plan_of(T, n_pts: int, n_lev: int, t: tuple[bool, int], q: tuple[bool, int]) -> Plan:
    elem, V = np.dtype(T).itemsize, vec(T)
    lt, lq = column_route(*t, n_lev, V)[1], column_route(*q, n_lev, V)[1]
    return plan_of(lambda pt: geo_carve(pt, lt, lq, elem, n_lev), n_pts)


def geo_plan(T, shape, storage="columns") -> Plan:
    """``shape``: (n_lev, kind, n_pts, with_zs), as ``geopotential_restatement.SHAPES``; ``storage``: one string for both stacks, or
    ``dict(t=, q=)``."""
    n_lev, _, n_pts, _ = shape
    kinds = storage if isinstance(storage, dict) else dict(t=storage, q=storage)
    return geo_plan_of(T, n_pts, n_lev, storage_form(kinds["t"], n_lev, T), storage_form(kinds["q"], n_lev, T))


# ---- csrc/heights/atx_heights.hip -------------------------------------------------------------------------------------------------
def window_bound(count: int, n_lev: int, V: int) -> int:
    """The elements the staged window of ``count`` variables covers at most: from the vector that holds its first row to the one that
    holds its last."""
    return (count * n_lev + 2 * (V - 1)) // V * V


def heights_carve(pt: int, lt: int, lq: int, elem: int, n_lev: int, n_tgt: int, x_least: int) -> tuple[int, int]:
    """``(total, x_bytes)``.  The x region starts the carve: what is dead once c is there (float64: the staged q columns; float32: the
    staged t and q columns and the delta terms), one variable's window at least; then the alpha terms (float64: the staged t columns),
    sp, z0, the brackets' w, a and b, the flags and the two coefficients of the n_lev + 1 half levels."""
    if elem == 8:
        end = round16(pt * lq * 8)
    else:
        odd = n_lev | 1
        end = round16(pt * lt * elem) + round16(pt * lq * elem) + round16(pt * odd * 8)
    x_bytes = max(end, round16(pt * x_least * elem))
    total = x_bytes + (round16(pt * lt * 8) if elem == 8 else round16(pt * (n_lev | 1) * 8))
    total += round16(pt * 8) + round16(pt * 8)
    total += round16(pt * n_tgt * 8) + round16(pt * n_tgt * 4) + round16(pt * n_tgt * 4)
    total += round16(pt * 4)
    total += round16(2 * (n_lev + 1) * 8)
    return total, x_bytes


def heights_chunk(PT: int, x_bytes: int, elem: int, n_lev: int, n_var: int, vx: int) -> int:
    """The variables the x region holds at a time: one at least."""
    chunk = 1
    while chunk < n_var and PT * window_bound(chunk + 1, n_lev, vx) * elem <= x_bytes:
        chunk += 1
    return chunk


def heights_plan_of(T, n_pts: int, n_lev: int, n_tgt: int, n_var: int, src: tuple[bool, int], t: tuple[bool, int], q: tuple[bool, int]) -> Plan:
    elem, V = np.dtype(T).itemsize, vec(T)
    lt, lq = column_route(*t, n_lev, V)[1], column_route(*q, n_lev, V)[1]
    vx = V if column_route(*src, n_var * n_lev, V)[0] else 1
    carve = lambda pt: heights_carve(pt, lt, lq, elem, n_lev, n_tgt, window_bound(1, n_lev, vx))  # noqa: E731
    return plan_of(lambda pt: carve(pt)[0], n_pts, lambda PT: heights_chunk(PT, carve(PT)[1], elem, n_lev, n_var, vx))


MIXED_HEIGHTS = dict(src="columns-base+1", t="columns", q="columns-pitch+1")  # test_gpu_heights.MIXED
MIXED_GEOPOTENTIAL = dict(t="columns", q="columns-pitch+1")                   # "columns-t-aligned-q-pitch+1" of test_gpu_geopotential


def heights_plan(T, shape, storage="columns") -> Plan:
    """``shape``: (n_pts, n_lev, kind, n_tgt, n_var, reference), as ``heights_restatement.SHAPES``; ``storage``: one string for the
    three stacks, or ``dict(src=, t=, q=)``."""
    n_pts, n_lev, _, n_tgt, n_var, _ = shape
    kinds = storage if isinstance(storage, dict) else dict(src=storage, t=storage, q=storage)
    return heights_plan_of(T, n_pts, n_lev, n_tgt, n_var, storage_form(kinds["src"], n_var * n_lev, T), storage_form(kinds["t"], n_lev, T),
                           storage_form(kinds["q"], n_lev, T))


PLANS = {LEVELS: levels_plan, GEOPOTENTIAL: geo_plan, HEIGHTS: heights_plan}


def points_of(kernel: str, shape) -> int:
    return shape[2] if kernel == GEOPOTENTIAL else shape[0]


# ---- searches along one axis -------------------------------------------------------------------------------------------------------
def first_refused(plan_at, start: int = 1, stop: int = 65536) -> int:
    """The smallest n in [start, stop) whose ``plan_at(n)`` is refused; the plans are accepted below it (one point's bytes grow with n)."""
    lo, hi = start, stop
    assert not plan_at(lo).refused and plan_at(hi - 1).refused
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if plan_at(mid).refused else (mid, hi)
    return hi


LEVELS_BOUNDARY = dict(n_lev=137, n_tgt=13)  # the axis is n_var
HEIGHTS_BOUNDARY = dict(n_lev=3)             # the axis is n_tgt


def levels_first_refused(T, storage: str = "columns", n_pts: int = 9) -> int:
    """The smallest refused n_var at 137 levels and 13 targets (n_var x n_lev stays inside the 65 535 rows of one launch)."""
    return first_refused(lambda n_var: levels_plan(T, (n_pts, LEVELS_BOUNDARY["n_lev"], LEVELS_BOUNDARY["n_tgt"], n_var), storage), 1, 65535 // 137)


def heights_first_refused(T, storage="columns", n_pts: int = 9) -> int:
    """The smallest refused n_tgt at 3 levels, one variable."""
    return first_refused(lambda n_tgt: heights_plan(T, (n_pts, HEIGHTS_BOUNDARY["n_lev"], WHOLE, n_tgt, 1, GROUND), storage), 1, 65536)


# ---- the cases of the GPU test, by regime ------------------------------------------------------------------------------------------
CAP, SMALL, WIDE, LARGEST, CHUNKS = "cap", "small-tile", "64KiB", "largest-accepted", "chunks"


class TileCase(NamedTuple):
    kernel: str
    T: type
    shape: tuple
    storages: tuple          # every storage the GPU test runs the case in: each must land in the regime
    regime: str
    PT: int                  # expected, in every storage
    budget: int
    last: int                # the points of the last tile
    chunk: object = None         # heights alone: the variables staged at a time; a tuple: per storage
    coordinate: str = "linear"   # levels alone

    @property
    def name(self) -> str:
        return f"{self.kernel}-{np.dtype(self.T).name}-{self.regime}-" + "x".join(str(v) for v in self.shape) + ("-log" if self.coordinate == "log" else "")


HEIGHTS_STORAGE = COLUMN_STORAGE + ("mixed",)
GEOPOTENTIAL_STORAGE = COLUMN_STORAGE + ("mixed",)


def storage_of(kernel: str, storage: str):
    """What the plan functions take for a storage name of a case: "mixed" is the kernel's mixed form."""
    if storage != "mixed":
        return storage
    return MIXED_HEIGHTS if kernel == HEIGHTS else MIXED_GEOPOTENTIAL


def _cases() -> tuple:
    f32, f64 = np.float32, np.float64
    L = lambda n_var, n_pts=9: (n_pts, 137, 13, n_var)  # noqa: E731
    H = lambda n_tgt, reference, n_lev=3, n_var=1, n_pts=9: (n_pts, n_lev, WHOLE, n_tgt, n_var, reference)  # noqa: E731
    top = {T: levels_first_refused(T) - 1 for T in (f32, f64)}
    most = {T: heights_first_refused(T) - 1 for T in (f32, f64)}
    out = []
    # the cap: PT = 256, more than one tile, a last tile of 1 and of 255 points
    for T in (f32, f64):
        out += [TileCase(LEVELS, T, (513, 2, 1, 1), COLUMN_STORAGE, CAP, 256, LDS_PREFERRED, 1),
                TileCase(LEVELS, T, (511, 2, 1, 1), COLUMN_STORAGE, CAP, 256, LDS_PREFERRED, 255),
                TileCase(HEIGHTS, T, (513, 2, WHOLE, 1, 1, SEA), HEIGHTS_STORAGE, CAP, 256, LDS_PREFERRED, 1, 1),
                TileCase(HEIGHTS, T, (511, 2, WHOLE, 1, 1, GROUND), HEIGHTS_STORAGE, CAP, 256, LDS_PREFERRED, 255, 1),
                TileCase(GEOPOTENTIAL, T, (2, WHOLE, 511, True), GEOPOTENTIAL_STORAGE, CAP, 256, LDS_PREFERRED, 255)]
    # tiles of one to four points under the preferred budget: 137 levels to 13 targets, a 9- or 10-point field ending on a one-point tile
    out += [TileCase(LEVELS, f64, L(12), COLUMN_STORAGE, SMALL, 1, LDS_PREFERRED, 1),
            TileCase(LEVELS, f64, L(5), COLUMN_STORAGE, SMALL, 4, LDS_PREFERRED, 1),
            TileCase(LEVELS, f32, L(12, 10), COLUMN_STORAGE, SMALL, 3, LDS_PREFERRED, 1),
            TileCase(LEVELS, f32, L(12, 10), COLUMN_STORAGE, SMALL, 3, LDS_PREFERRED, 1, None, "log"),
            TileCase(HEIGHTS, f32, H(300, GROUND, 137), HEIGHTS_STORAGE, SMALL, 3, LDS_PREFERRED, 3, 1),
            TileCase(HEIGHTS, f64, H(300, SEA, 137), HEIGHTS_STORAGE, SMALL, 4, LDS_PREFERRED, 1, 1),
            TileCase(HEIGHTS, f32, H(1500, GROUND), HEIGHTS_STORAGE, SMALL, 1, LDS_PREFERRED, 1, 1),
            TileCase(HEIGHTS, f64, H(1500, SEA), HEIGHTS_STORAGE, SMALL, 1, LDS_PREFERRED, 1, 1)]
    # one point does not fit 32 KiB: the 64 KiB budget, up to the largest shape that is accepted
    out += [TileCase(LEVELS, f64, L(25), COLUMN_STORAGE, WIDE, 2, LDS_LIMIT, 1),
            TileCase(LEVELS, f64, L(29), COLUMN_STORAGE, WIDE, 1, LDS_LIMIT, 1),
            TileCase(LEVELS, f64, L(29), COLUMN_STORAGE, WIDE, 1, LDS_LIMIT, 1, None, "log"),
            TileCase(LEVELS, f64, L(top[f64]), COLUMN_STORAGE, LARGEST, 1, LDS_LIMIT, 1),
            TileCase(LEVELS, f32, L(top[f32]), COLUMN_STORAGE, LARGEST, 1, LDS_LIMIT, 1)]
    for T, reference in ((f32, SEA), (f64, GROUND)):
        out += [TileCase(HEIGHTS, T, H(3000, reference), HEIGHTS_STORAGE, WIDE, 1, LDS_LIMIT, 1, 1),
                TileCase(HEIGHTS, T, H(most[T], reference), HEIGHTS_STORAGE, LARGEST, 1, LDS_LIMIT, 1, 1)]
    # the variables staged a chunk at a time, the chunk at most a third of them; n_lev is odd: a later chunk's first row is not the
    # first element of its window on the 16-byte route (float32: 4 x 137 is a whole number of vectors, 3 x 135 is not)
    out += [TileCase(HEIGHTS, f32, (10, 135, WHOLE, 13, 13, GROUND), HEIGHTS_STORAGE, CHUNKS, 8, LDS_PREFERRED, 2, (3, 4, 4, 4)),
            TileCase(HEIGHTS, f64, (10, 137, WHOLE, 13, 7, SEA), HEIGHTS_STORAGE, CHUNKS, 12, LDS_PREFERRED, 10, 1)]
    return tuple(out)


TILE_CASES = _cases()
