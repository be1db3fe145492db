"""The checks that hold the reduction and mask kernels (csrc/atx_reduce.hip, csrc/atx_mask.hip), the index guard ``atx_check_indices``
and ``atx_stream_copy`` to numpy — written once, as plain functions over the callables under test and a device.
tests/test_gpu_reduce_mask_edges.py runs them on ``native.*`` on an MI355X; tests/test_reduce_mask_checks_catch_defects.py runs them on
the CPU against a numpy stand-in, once as it is and once per planted defect.

Every reference is an exact numpy operation on the host — ``np.min`` / ``np.max`` (both propagate NaN), ``np.isnan(x).sum()``, the
comparison ufuncs on arrays of the STORED dtype, ``np.count_nonzero``, ``np.flatnonzero`` — so every assertion is equality; no
tolerance appears.  (``np.min`` is taken in the stored dtype and the result widened: widening is monotonic and exact, so this IS the
minimum of the widened inputs, without a float64 copy of the large shapes.)  The one case numpy does not fix is an extreme attained by
both ``+0.0`` and ``-0.0`` (its answer depends on its SIMD order): compared with ``==``; where ``-0.0`` alone attains it, bit patterns.

What numpy does for ``float32_array > 0.1`` (numpy 2.2.6, NEP 50): the Python float is "weak", it is converted to the array's
float32 and the comparison runs in float32 — ``a > 0.1`` equals ``a > np.float32(0.1)`` and differs from the float64 comparison
``a.astype(np.float64) > 0.1`` exactly at ``a == np.float32(0.1)`` (which is above the double 0.1).  numpy 1.x's value-based casting
gave the same float32 comparison.  That is the kernel's ``(float)threshold``, and the statement of R: apply_mask.py:160-163 on float32
``mask_values``: nothing to reconcile.  ``test_reduce_mask_checks_catch_defects.py::test_numpy_compares_a_float32_field_in_float32`` pins it.

The sizes "past the cap" are derived from the kernels' own constants, read from the sources below at import time.
"""

from __future__ import annotations

import math
import os
import re
import struct
import zlib
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

from anemoi_transform_amd import native

COLUMNS, FIELDS = native.COLUMNS, native.FIELDS
REDS = (native.RED_MIN, native.RED_MAX, native.RED_MINMAX, native.RED_NANCOUNT)
RED_NAMES = {native.RED_MIN: "MIN", native.RED_MAX: "MAX", native.RED_MINMAX: "MINMAX", native.RED_NANCOUNT: "NANCOUNT"}
CMPS = {"GT": native.CMP_GT, "LT": native.CMP_LT, "EQ": native.CMP_EQ, "NE": native.CMP_NE, "GE": native.CMP_GE, "LE": native.CMP_LE,
        "NOTNAN": native.CMP_NOTNAN, "ISNAN": native.CMP_ISNAN}
UFUNCS = {"GT": np.greater, "LT": np.less, "EQ": np.equal, "NE": np.not_equal, "GE": np.greater_equal, "LE": np.less_equal}
THRESHOLDS = (0.0, -0.0, 0.1, 1e-5, math.inf, -math.inf, math.nan)
DTYPES = (np.float32, np.float64)
NAN = float("nan")


# ---- the kernels' constants ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Constants:
    block: int        # kBlock: lanes per workgroup
    wave: int         # kWave
    red_grid: int     # kRedGrid: workgroup cap of the reductions = partial slots of their workspace
    red_unroll: int   # kRedUnroll: items per lane and sweep
    stream_grid: int  # kStreamGrid: workgroup cap of the grid-stride streaming kernels (mask_build, check_indices)
    per_lane: int     # kPerLane: mask bytes per lane of the compaction
    count_grid: int   # workgroup clamp of mask_count
    self_scan: int    # kCompactSelfScan: workgroups up to which the scatter sums the counts before it by itself

    @property
    def chunk(self) -> int:  # kChunk: mask bytes per workgroup of the compaction
        return self.block * self.per_lane

    def sweep_items(self, tail: bool = False) -> int:
        """Items the capped reduction grid takes in ONE sweep (a flat array's tail takes one workspace slot: the cap is one less)."""
        return (self.red_grid - (1 if tail else 0)) * self.block * self.red_unroll


def read_constants() -> Constants:
    csrc = os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc")

    def find(name, pattern):
        with open(os.path.join(csrc, name)) as f:
            m = re.search(pattern, f.read())
        assert m, f"{name}: {pattern} not found"
        return int(m.group(1))

    return Constants(
        block=find("atx_common.hpp", r"constexpr int kBlock = (\d+);"),
        wave=find("atx_common.hpp", r"constexpr int kWave = (\d+);"),
        red_grid=find("atx_reduce.hip", r"constexpr int64_t kRedGrid = (\d+);"),
        red_unroll=find("atx_reduce.hip", r"constexpr int kRedUnroll = (\d+);"),
        stream_grid=find("atx_common.hpp", r"#define ATX_MAX_GRID (\d+)"),
        per_lane=find("atx_mask.hip", r"constexpr int kPerLane = (\d+);"),
        count_grid=find("atx_mask.hip", r"count_grid = grid_for\(n\) > (\d+)u"),
        self_scan=find("atx_mask.hip", r"constexpr int kCompactSelfScan = (\d+);"),
    )


K = read_constants()


@dataclass
class Kernels:
    """The callables under test, with the signatures of ``native.reduce`` ... ``native.stream_copy``.  ``use_workspace(flag)`` picks the
    reductions' route (``native._REDUCE_TICKET``); ``index_into(mask, n, index) -> count`` is ``atx_mask_to_index`` into a caller's
    buffer (``native.mask_to_index`` allocates its own, which no canary can follow)."""

    reduce: Callable
    reduce_stack: Callable
    mask_build: Callable
    mask_count: Callable
    mask_to_index: Callable
    index_into: Callable
    check_indices: Callable
    stream_copy: Callable
    use_workspace: Callable


# ---- storage shapes of the reductions -----------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Shape:
    """``n_rows`` rows of ``row_len`` elements ``pitch`` apart, ``offset`` elements into a larger allocation.  kind "flat": one row
    through ``reduce``; "columns": rows are points, ``row_len`` levels; "fields": rows are levels, ``row_len`` points."""

    name: str
    np_dtype: type
    kind: str
    n_rows: int
    row_len: int
    pitch: int
    offset: int = 0
    poison: str = "nan"  # what the padding and the elements around the buffer hold: "nan", or "beyond" (±1e30 alternating)

    @property
    def vec(self) -> int:
        return 4 if self.np_dtype == np.float32 else 2

    @property
    def tail(self) -> int:
        return self.row_len % self.vec if (self.n_rows == 1 and self.offset == 0) else 0

    def route(self) -> str:
        """reduce_rows' choice: 16-byte loads when the base is aligned and every row's last vector lies inside an aligned pitch."""
        body = self.row_len - self.tail
        c = -(-body // self.vec)
        ok = self.offset == 0 and (self.n_rows == 1 or (self.pitch % self.vec == 0 and c * self.vec <= self.pitch))
        return "16-byte" if ok else "scalar"

    def n_items(self) -> int:
        """What the grid is sized by: (row, vector) pairs on the 16-byte route, elements on the scalar one."""
        if self.route() == "16-byte":
            return self.n_rows * (-(-(self.row_len - self.tail) // self.vec))
        return self.n_rows * self.row_len

    def item_elements(self, item: int):
        """(row, first column, last column) of an item."""
        if self.route() == "16-byte":
            body = self.row_len - self.tail
            c = -(-body // self.vec)
            r, cv = divmod(item, c)
            return r, cv * self.vec, min(cv * self.vec + self.vec, body) - 1
        r, col = divmod(item, self.row_len)
        return r, col, col


def torch_dtype(np_dtype):
    return torch.float32 if np_dtype == np.float32 else torch.float64


class Storage:
    def __init__(self, shape: Shape, device, values: Optional[np.ndarray] = None):
        s = self.shape = shape
        n = s.n_rows * s.pitch
        guard = 2 * s.vec
        total = n + s.offset + guard
        if s.poison == "nan":
            self.backing = torch.full((total,), NAN, dtype=torch_dtype(s.np_dtype), device=device)
        else:
            sign = 1.0 - 2.0 * (torch.arange(total, device=device) % 2).to(torch_dtype(s.np_dtype))
            self.backing = sign * 1e30
        assert self.backing.data_ptr() % 16 == 0
        self.flat = self.backing[s.offset: s.offset + n]
        self.view2d = self.flat.view(s.n_rows, s.pitch)
        assert (self.flat.data_ptr() % 16 == 0) == (s.offset == 0)
        if values is not None:
            self.view2d[:, : s.row_len] = torch.from_numpy(np.ascontiguousarray(values)).to(device)

    def put(self, r: int, c: int, v) -> None:
        self.view2d[r, c] = float(v)


def call(kern: Kernels, st: Storage, red: int):
    s = st.shape
    if s.kind == "flat":
        return kern.reduce(st.flat, red, s.row_len)
    if s.kind == "columns":
        return kern.reduce_stack(st.view2d, red, n_pts=s.n_rows, n_lev=s.row_len, pitch=s.pitch, layout=COLUMNS)
    return kern.reduce_stack(st.view2d, red, n_pts=s.row_len, n_lev=s.n_rows, pitch=s.pitch, layout=FIELDS)


def reference(vals: np.ndarray) -> dict:
    with np.errstate(all="ignore"):
        mn, mx = float(np.min(vals)), float(np.max(vals))  # widened after the fact: exact (module docstring)
        cnt = float(np.isnan(vals).sum())
    return {native.RED_MIN: mn, native.RED_MAX: mx, native.RED_MINMAX: (mn, mx), native.RED_NANCOUNT: cnt}


def closed_form(mn: float, mx: float, cnt: float) -> dict:
    return {native.RED_MIN: mn, native.RED_MAX: mx, native.RED_MINMAX: (mn, mx), native.RED_NANCOUNT: float(cnt)}


def same(a, b, bits: bool = False) -> bool:
    if isinstance(b, tuple):
        return isinstance(a, tuple) and len(a) == len(b) and all(same(x, y, bits) for x, y in zip(a, b))
    if isinstance(a, tuple):
        return False
    if math.isnan(b):
        return math.isnan(a)
    if bits:
        return struct.pack("<d", a) == struct.pack("<d", b)
    return a == b


def check_reductions(kern: Kernels, st: Storage, want: dict, check: str, label: str, repeats: int = 3, bits: bool = False, reds=REDS):
    """Each reduction with and without the workspace, ``repeats`` calls in a row on the reused workspace: each equals numpy, and
    the two routes equal each other."""
    seen = {}
    try:
        for ws in (True, False):
            kern.use_workspace(ws)
            for red in reds:
                for i in range(repeats):
                    got = call(kern, st, red)
                    assert same(got, want[red], bits), (
                        f"{check}: {label} [{st.shape.route()} route, {'workspace' if ws else 'atomics'}] {RED_NAMES[red]} call {i + 1}: "
                        f"kernel {got!r}, numpy {want[red]!r}")
                seen[ws, red] = got
    finally:
        kern.use_workspace(True)
    for red in reds:
        assert same(seen[True, red], seen[False, red], bits), (
            f"routes disagree: {label} {RED_NAMES[red]}: workspace {seen[True, red]!r}, atomics {seen[False, red]!r}")


def roundup(n: int, m: int) -> int:
    return -(-n // m) * m


def small_shapes(np_dtype) -> list:
    """Both layouts, ``row_len`` 1..9 (both sides of every multiple of the vector width), pitches tight / aligned / odd / aligned but
    wider than a vector, padding poisoned with NaN and with values beyond both extremes, and a base one element off."""
    vec = 4 if np_dtype == np.float32 else 2
    t = "f32" if np_dtype == np.float32 else "f64"
    out = []
    for kind in ("columns", "fields"):
        for row_len in range(1, 10):
            al = roundup(row_len, vec)
            out.append(Shape(f"{t}-{kind}-len{row_len}-tight", np_dtype, kind, 3, row_len, row_len))
            for pname, pitch in (("aligned", al), ("odd", al + 1), ("wide", al + 2 * vec)):
                for poison in ("nan", "beyond"):
                    out.append(Shape(f"{t}-{kind}-len{row_len}-{pname}{pitch}-{poison}", np_dtype, kind, 3, row_len, pitch, 0, poison))
            out.append(Shape(f"{t}-{kind}-len{row_len}-aligned{al}-base1", np_dtype, kind, 3, row_len, al, 1, "nan"))
    return out


def mid_shapes(np_dtype, k: Constants = K) -> list:
    """Stacks of several workgroups' shares (a 137-level column stack, a 5-level field stack) on both routes."""
    vec = 4 if np_dtype == np.float32 else 2
    t = "f32" if np_dtype == np.float32 else "f64"
    share = k.block * k.red_unroll
    al = roundup(137, vec)
    rows = 3 * share // (al // vec) + 2
    n_pts = share * vec * 2 + 3
    return [
        Shape(f"{t}-columns-137x{rows}-aligned{al}-nan", np_dtype, "columns", rows, 137, al, 0, "nan"),
        Shape(f"{t}-columns-137x{rows}-wide{al + 2 * vec}-beyond", np_dtype, "columns", rows, 137, al + 2 * vec, 0, "beyond"),
        Shape(f"{t}-columns-137x{rows}-odd{al + 1}-nan", np_dtype, "columns", rows, 137, al + 1, 0, "nan"),
        Shape(f"{t}-columns-137x{rows}-aligned{al}-base1", np_dtype, "columns", rows, 137, al, 1, "nan"),
        Shape(f"{t}-fields-5x{n_pts}-aligned{roundup(n_pts, vec)}-nan", np_dtype, "fields", 5, n_pts, roundup(n_pts, vec), 0, "nan"),
        Shape(f"{t}-fields-5x{n_pts}-tight", np_dtype, "fields", 5, n_pts, n_pts, 0, "beyond"),
    ]


def flat_shapes(np_dtype, k: Constants = K) -> list:
    """Flat arrays: nothing but a tail, every tail residue, around one workgroup's share, and several hundred workgroups (more
    partials than the finishing workgroup has lanes) — from an aligned base and from one element off."""
    vec = 4 if np_dtype == np.float32 else 2
    t = "f32" if np_dtype == np.float32 else "f64"
    share = k.block * k.red_unroll * vec
    many = share * (k.block + 37)  # > kBlock partials through reduce_final_kernel
    out = []
    for n in list(range(1, 10)) + [share - 1, share, share + 1, many + 1, many + vec - 1]:
        out.append(Shape(f"{t}-flat-{n}", np_dtype, "flat", 1, n, n))
    for n in (1, 5, share + 1, many // 4 + 1):
        out.append(Shape(f"{t}-flat-{n}-base1", np_dtype, "flat", 1, n, n, 1))
    return out


def walk_positions(s: Shape, k: Constants = K) -> dict:
    """The structurally distinct places of a shape: (row, col) -> what it is."""
    pos = {}

    def add(name, r, c):
        if 0 <= r < s.n_rows and 0 <= c < s.row_len:
            pos.setdefault((r, c), name)

    last_r, body = s.n_rows - 1, s.row_len - s.tail
    for r, rn in ((0, "first row"), (last_r, "last row")):
        add(f"first element of the {rn}", r, 0)
        add(f"last element of the {rn}", r, s.row_len - 1)
        if body > 0:
            for c in range((body - 1) // s.vec * s.vec, body):
                add(f"element {c % s.vec} of the last vector of the {rn}", r, c)
    for c in range(body, s.row_len):
        add(f"tail element {c - body}", 0, c)
    n_items = s.n_items()
    if n_items > 0:
        cap = k.red_grid - (1 if s.tail else 0)
        grid = min(cap, max(1, -(-n_items // (k.block * k.red_unroll))))
        stride = grid * k.block
        sweep = stride * k.red_unroll
        marks = {"a wave's lanes": k.wave, "a wave's share": k.wave * k.red_unroll, "a workgroup's lanes": k.block,
                 "a workgroup's share": k.block * k.red_unroll, "the grid's stride": stride, "the last workgroup": (grid - 1) * k.block,
                 "the last item": n_items}
        for j in range(1, min(4, -(-n_items // sweep)) + 1):
            marks[f"sweep {j}"] = min(j * sweep, n_items)
        for name, m in marks.items():
            for item, side in ((m - 1, "before the end of"), (m, "after")):
                if 0 <= item < n_items:
                    r, c0, c1 = s.item_elements(item)
                    add(f"first element of the item {side} {name}", r, c0)
                    add(f"last element of the item {side} {name}", r, c1)
        rng = np.random.default_rng(zlib.crc32(s.name.encode()))
        for item in rng.integers(0, n_items, size=4):
            r, c0, c1 = s.item_elements(int(item))
            add(f"seeded item {int(item)}", r, c1)
    return pos


def check_walked_positions(kern: Kernels, device, s: Shape, k: Constants = K, repeats: int = 3) -> int:
    """A constant field; the single extreme (one float below, one float above the constant), then the single NaN, at each
    structurally distinct position in turn.  Returns the number of positions walked."""
    const = s.np_dtype(0.1) * s.np_dtype(3)  # not a round number in either width
    low, high = np.nextafter(const, s.np_dtype(-np.inf)), np.nextafter(const, s.np_dtype(np.inf))
    vals = np.full((s.n_rows, s.row_len), const, dtype=s.np_dtype)
    st = Storage(s, device, vals)
    positions = walk_positions(s, k)
    label = f"{s.name} ({len(positions)} positions walked)"
    check_reductions(kern, st, reference(vals), "walked extreme", f"{label}: the constant field", repeats)
    for (r, c), name in positions.items():
        for what, v in (("the minimum", low), ("the maximum", high), ("the NaN", s.np_dtype(np.nan))):
            vals[r, c] = v
            st.put(r, c, v)
            want = reference(vals)
            if what == "the NaN":
                assert same(want[native.RED_MINMAX], (NAN, NAN)) and want[native.RED_NANCOUNT] == 1.0
            check_reductions(kern, st, want, "walked NaN" if what == "the NaN" else "walked extreme",
                             f"{label}: {what} at the {name} (row {r}, col {c})", repeats)
        vals[r, c] = const
        st.put(r, c, const)
    return len(positions)


def special_cases(s: Shape) -> list:
    """(name, values, compare bit patterns)"""
    dt = s.np_dtype
    rng = np.random.default_rng(zlib.crc32(("special " + s.name).encode()))
    shape = (s.n_rows, s.row_len)
    n = s.n_rows * s.row_len
    finite = (10.0 * rng.standard_normal(shape)).astype(dt)
    positive = (np.abs(finite) + dt(1)).astype(dt)
    unit = rng.uniform(0.2, 0.9, shape).astype(dt)
    info = np.finfo(dt)
    sub = info.smallest_subnormal

    def with_values(base, *vs):
        a = base.copy()
        spots = rng.choice(n, size=min(n, len(vs)), replace=False)
        for spot, v in zip(spots, vs):
            a[np.unravel_index(int(spot), shape)] = dt(v)
        return a

    cases = [
        ("finite data", finite, False),
        ("all +inf", np.full(shape, np.inf, dt), False),
        ("all -inf", np.full(shape, -np.inf, dt), False),
        ("all NaN", np.full(shape, np.nan, dt), False),
        ("+inf among finite data", with_values(finite, np.inf), False),
        ("-inf among finite data", with_values(finite, -np.inf), False),
        ("both infinities among finite data", with_values(finite, np.inf, -np.inf), False),
        ("the largest finite numbers", with_values(finite, info.max, -info.max), False),
        ("-0.0 the only non-positive value", with_values(positive, -0.0), n >= 1),
        ("-0.0 the only non-negative value", with_values(-positive, -0.0), n >= 1),
        ("-0.0 and +0.0 both attain the minimum", with_values(positive, -0.0, 0.0), False),  # numpy's pick depends on its SIMD order: ==
        ("-0.0 and +0.0 both attain the maximum", with_values(-positive, 0.0, -0.0), False),
        ("a subnormal minimum", with_values(positive, sub), True),
        ("a subnormal maximum", with_values(-positive, -sub), True),
        ("subnormals of both signs around zero", with_values(np.zeros(shape, dt), sub, -sub, 3 * sub), n >= 3),
        ("extremes that are no round float64 numbers", with_values(unit, dt(0.1), np.nextafter(dt(1), dt(2))), True),
        ("one NaN", with_values(finite, np.nan), False),
    ]
    some = finite.copy()
    some[rng.random(shape) < 0.37] = np.nan
    cases.append(("a seeded 37 % NaN", some, False))
    return cases


def check_special_values(kern: Kernels, device, s: Shape, repeats: int = 3) -> None:
    for name, vals, bits in special_cases(s):
        st = Storage(s, device, vals)
        want = reference(vals)
        if name == "extremes that are no round float64 numbers" and vals.size >= 2:
            assert want[native.RED_MINMAX] == (float(s.np_dtype(0.1)), float(np.nextafter(s.np_dtype(1), s.np_dtype(2))))
        check_reductions(kern, st, want, "special values", f"{s.name}: {name}", repeats, bits=bits)


# ---- past the workgroup cap ---------------------------------------------------------------------------------------------------
def past_cap_shapes(k: Constants = K) -> list:
    """(shape, check a host copy too).  Every shape has two full sweeps of the capped grid and an odd remainder."""
    out = []
    rem = k.block * k.red_unroll * 37 + 13
    for dt, t in ((np.float32, "f32"), (np.float64, "f64")):
        vec = 4 if dt == np.float32 else 2
        for tail in ((1, 3) if vec == 4 else (1,)):
            n = (2 * k.sweep_items(True) + rem) * vec + tail
            out.append((Shape(f"{t}-flat-{n}-tail{tail}", dt, "flat", 1, n, n), False))
        sweep = k.sweep_items()
        al = roundup(137, vec)
        c = al // vec
        assert c % 2 == 1
        rows = -(-(2 * sweep + rem) // c) | 1
        out.append((Shape(f"{t}-columns-137x{rows}-aligned{al}", dt, "columns", rows, 137, al), False))
        c = -(-(2 * sweep + rem) // 3) | 1
        out.append((Shape(f"{t}-fields-3x{c * vec - 1}-aligned{c * vec}", dt, "fields", 3, c * vec - 1, c * vec), False))
        n = 2 * sweep + rem
        out.append((Shape(f"{t}-flat-{n}-base1", dt, "flat", 1, n, n, 1), dt == np.float32))
        rows = -(-n // 137) | 1
        out.append((Shape(f"{t}-columns-137x{rows}-odd{al + 1}", dt, "columns", rows, 137, al + 1), dt == np.float32))
        n_pts = -(-n // 3) | 1
        out.append((Shape(f"{t}-fields-3x{n_pts}-odd{n_pts + 2}", dt, "fields", 3, n_pts, n_pts + 2), False))
    return out


def fill_closed_form(st: Storage, period: int) -> None:
    """element (r, c) = (r * row_len + c) mod period, built on the device in pieces."""
    s = st.shape
    piece = 1 << 24
    dev, td = st.backing.device, st.backing.dtype
    if s.n_rows == 1:
        for c0 in range(0, s.row_len, piece):
            c1 = min(s.row_len, c0 + piece)
            st.view2d[0, c0:c1] = torch.arange(c0, c1, device=dev, dtype=torch.int64).remainder_(period).to(td)
        return
    per = max(1, piece // s.row_len)
    for r0 in range(0, s.n_rows, per):
        r1 = min(s.n_rows, r0 + per)
        idx = torch.arange(r0 * s.row_len, r1 * s.row_len, device=dev, dtype=torch.int64).remainder_(period)
        st.view2d[r0:r1, : s.row_len] = idx.view(r1 - r0, s.row_len).to(td)


def check_past_the_cap(kern: Kernels, device, s: Shape, k: Constants = K, host_copy: bool = False) -> dict:
    """Closed-form data (extremes and NaN count known without a host pass) over more than two sweeps of the capped grid; then a
    second extreme of each kind and one NaN at the first and last element of EVERY sweep and in the tail.  Returns the sizes."""
    n_items, sweep = s.n_items(), k.sweep_items(s.tail > 0)
    assert sweep == (k.red_grid - (1 if s.tail else 0)) * k.block * k.red_unroll
    beyond = n_items - sweep
    assert beyond >= sweep + 1 and (beyond - sweep) % 2 == 1, (
        f"past the cap: {s.name} has {n_items} items on the {s.route()} route; needs {sweep} + a full sweep + an odd remainder")
    n_elem = s.n_rows * s.row_len
    period = min(999983, n_elem // 3)  # exact in float32, and every value occurs at least twice
    st = Storage(s, device)
    fill_closed_form(st, period)
    label = f"{s.name} ({n_items} items > {sweep})"
    base = closed_form(0.0, float(period - 1), 0)
    check_reductions(kern, st, base, "past the cap", f"{label}: closed form", repeats=3)
    low, high = -3.0, float(period + 11)
    spots = {}
    n_sweeps = -(-n_items // sweep)
    assert n_sweeps >= 3
    for j in range(n_sweeps):
        r, c0, _ = s.item_elements(j * sweep)
        spots.setdefault((r, c0), f"first element of sweep {j + 1}")
        r, _, c1 = s.item_elements(min((j + 1) * sweep, n_items) - 1)
        spots.setdefault((r, c1), f"last element of sweep {j + 1}")
    for c in range(s.row_len - s.tail, s.row_len):
        spots.setdefault((0, c), f"tail element {c - (s.row_len - s.tail)}")
    for (r, c), name in spots.items():
        old = float(st.view2d[r, c])
        for what, v, want in (("a second minimum", low, closed_form(low, float(period - 1), 0)),
                              ("a second maximum", high, closed_form(0.0, high, 0)),
                              ("one NaN", NAN, closed_form(NAN, NAN, 1))):
            st.put(r, c, v)
            check_reductions(kern, st, want, "past the cap", f"{label}: {what} at the {name} ({len(spots)} positions walked)", repeats=1)
        st.put(r, c, old)
    if host_copy:
        (r, c), name = next((rc, nm) for rc, nm in spots.items() if nm == f"last element of sweep {n_sweeps}")
        st.put(r, c, low)
        vals = st.view2d[:, : s.row_len].cpu().numpy()
        want = reference(vals)
        for red in REDS:
            assert same(want[red], closed_form(low, float(period - 1), 0)[red]), f"past the cap: {label}: closed form differs from numpy on the host copy"
        check_reductions(kern, st, want, "past the cap", f"{label}: numpy on a host copy, a second minimum at the {name}", repeats=1)
    return {"shape": s.name, "route": s.route(), "items": n_items, "threshold": sweep, "bytes": st.backing.numel() * st.backing.element_size()}


# ---- masks --------------------------------------------------------------------------------------------------------------------
CANARY = 0xA5


def mask_field(np_dtype, threshold: float, n: int) -> np.ndarray:
    """NaN, ±inf, ±0.0, the threshold in the stored dtype and its two neighbours, subnormals and ordinary numbers, cycled to n."""
    dt = np_dtype
    with np.errstate(all="ignore"):
        thr = dt(threshold)
        sub = np.finfo(dt).smallest_subnormal
        pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, thr, np.nextafter(thr, dt(np.inf)), np.nextafter(thr, dt(-np.inf)), sub, -sub,
                         1.0, -1.0, 0.1, 1e-5, 2.5], dtype=dt)
    return np.resize(pool[np.random.default_rng(n).permutation(pool.size)] if n > pool.size else pool, n).astype(dt)


def mask_reference(field: np.ndarray, op: str, threshold: float) -> np.ndarray:
    """``numpy_ufunc(field_in_stored_dtype, stored_dtype(threshold))``"""
    with np.errstate(all="ignore"):
        if op == "NOTNAN":
            return ~np.isnan(field)
        if op == "ISNAN":
            return np.isnan(field)
        return UFUNCS[op](field, field.dtype.type(threshold))


def run_mask_build(kern: Kernels, device, field: np.ndarray, op: str, threshold: float, stride: int = 1, label: str = ""):
    """The level ``min(2, stride - 1)`` of a columns stack of pitch ``stride`` whose other levels are NaN; canary behind the mask."""
    n = field.size
    lev = min(2, stride - 1)
    stack = np.full((max(n, 1), stride), np.nan, dtype=field.dtype)
    stack[:n, lev] = field
    sd = torch.from_numpy(stack).to(device)
    m = sd.view(-1)[lev:]
    guard = 16
    mask = torch.full((roundup(n, 4) + guard,), CANARY, dtype=torch.uint8, device=device)
    kern.mask_build(m, mask, n=n, stride=stride, cmp=CMPS[op], threshold=threshold)
    got = mask.cpu().numpy()
    want = mask_reference(field, op, threshold).astype(np.uint8)
    what = f"mask_build: {label}{field.dtype.name} {op} {threshold!r}, n = {n}, m_stride = {stride}"
    bad = np.flatnonzero(got[:n] != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ from numpy, first at {bad[:5]}: field {field[bad[:5]]}, kernel {got[:n][bad[:5]]}, numpy {want[bad[:5]]}"
    assert np.all(got[n:] == CANARY), f"{what}: mask written past n at {n + np.flatnonzero(got[n:] != CANARY)[:5]}"
    assert np.array_equal(sd.cpu().numpy().view(np.uint8), stack.view(np.uint8)), f"{what}: the field was modified"


def mask_lengths(k: Constants = K) -> list:
    return list(range(10)) + [4095, 4096, 4097]


def check_mask_build(kern: Kernels, device, np_dtype, threshold: float, k: Constants = K) -> None:
    for op in CMPS:
        for n in mask_lengths(k):
            run_mask_build(kern, device, mask_field(np_dtype, threshold, n), op, threshold)
        for stride in (3, 137, 140):
            for n in (7, 4097):
                run_mask_build(kern, device, mask_field(np_dtype, threshold, n), op, threshold, stride, label="stride: ")


def check_mask_build_past_the_cap(kern: Kernels, device, np_dtype, k: Constants = K) -> int:
    cap = k.stream_grid * k.block * 4
    n = cap + k.block * 4 * 3 + 3
    assert n > cap
    for op, threshold in (("GT", 0.1), ("NE", 1e-5)):
        run_mask_build(kern, device, mask_field(np_dtype, threshold, n), op, threshold, label=f"past kStreamGrid x kBlock x 4 = {cap}: ")
    return n


def index_lengths(k: Constants = K) -> list:
    out = [0, 1]
    for edge in (k.chunk, k.count_grid * k.block, k.self_scan * k.chunk):
        out += [edge - 1, edge, edge + 1]
    return out


DENSITIES = ("none", "all", "0.37", "only the last byte")


def make_mask(n: int, density: str) -> np.ndarray:
    """Set bytes drawn from 1, 2, 128 and 255: any non-zero byte is set (include/atx.h: "non-zero mask bytes", "mask[i] != 0")."""
    rng = np.random.default_rng(zlib.crc32(f"mask {n} {density}".encode()))
    values = np.array([1, 2, 128, 255], dtype=np.uint8)[rng.integers(0, 4, size=n)]
    if density == "none":
        return np.zeros(n, dtype=np.uint8)
    if density == "all":
        return values
    if density == "0.37":
        return np.where(rng.random(n) < 0.37, values, 0).astype(np.uint8)
    out = np.zeros(n, dtype=np.uint8)
    out[-1:] = 255
    return out


INDEX_CANARY = -2147483641


def check_mask_count_and_index(kern: Kernels, device, n: int, density: str) -> None:
    host = make_mask(n, density)
    label = f"n = {n}, density {density}, bytes {sorted(set(host.tolist()))}"
    mask = torch.from_numpy(host).to(device) if n else torch.zeros(0, dtype=torch.uint8, device=device)
    want_count, want_index = int(np.count_nonzero(host)), np.flatnonzero(host).astype(np.int32)
    count = kern.mask_count(mask, n)
    assert count == want_count, f"mask_count: {label}: kernel {count}, numpy {want_count}"
    index = kern.mask_to_index(mask, n).cpu().numpy()
    assert index.dtype == np.int32 and index.size == want_count, f"index list: {label}: {index.size} entries, numpy {want_count}"
    bad = np.flatnonzero(index != want_index)
    assert bad.size == 0, f"index list: {label}: differs from np.flatnonzero at {bad[:5]}: kernel {index[bad[:5]]}, numpy {want_index[bad[:5]]}"
    buf = torch.full((n + 8,), INDEX_CANARY, dtype=torch.int32, device=device)
    got_count = kern.index_into(mask, n, buf)
    assert got_count == count, f"index list: {label}: count {got_count}, mask_count {count}"
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got[:want_count] != want_index)
    assert bad.size == 0, f"index list: {label}: differs from np.flatnonzero at {bad[:5]}: kernel {got[bad[:5]]}, numpy {want_index[bad[:5]]}"
    past = np.flatnonzero(got[want_count:] != INDEX_CANARY)
    assert past.size == 0, f"index list: {label}: written past index[count) at {want_count + past[:5]}"
    assert np.array_equal(mask.cpu().numpy(), host), f"index list: {label}: the mask was modified"


# ---- the index guard ----------------------------------------------------------------------------------------------------------
def check_indices_lengths(k: Constants = K) -> list:
    return [0, 1, 63, 64, 65, k.stream_grid * k.block + k.block + 1]


def check_check_indices(kern: Kernels, device, n: int, k: Constants = K) -> None:
    i32 = np.iinfo(np.int32)
    for n_src in (1000, 1):
        base = (np.arange(n, dtype=np.int64) % n_src).astype(np.int32)

        def run(table, label):
            want = int(((table < 0) | (table.astype(np.int64) >= n_src)).sum())
            got = kern.check_indices(torch.from_numpy(table).to(device) if n else torch.zeros(0, dtype=torch.int32, device=device), n_src)
            assert got == want, f"check_indices: n = {n}, n_src = {n_src}, {label}: kernel {got}, numpy {want}"

        run(base, "a valid table")
        places = sorted({p for p in (0, n - 1, k.block - 1, k.block, k.stream_grid * k.block - 1, k.stream_grid * k.block) if 0 <= p < n})
        for v in (-1, n_src, n_src - 1, 0, int(i32.min), int(i32.max)):
            for p in places:
                table = base.copy()
                table[p] = v
                run(table, f"{v} at {p}")
        if n > 1:
            rng = np.random.default_rng(n)
            table = base.copy()
            spots = rng.random(n) < 0.01
            table[spots] = rng.choice(np.array([-1, n_src, int(i32.min), int(i32.max), n_src + 1], dtype=np.int64), size=int(spots.sum())).astype(np.int32)
            table[-1] = n_src
            run(table, "a seeded 1 % of bad entries")


# ---- the reference streaming copy ---------------------------------------------------------------------------------------------
def stream_copy_sizes(k: Constants = K) -> list:
    """16, 32 and 4096 bytes and one size beyond kStreamGrid workgroups of 16 bytes per lane (the kernel takes one lane per 16 bytes
    with no cap: this pins that none is silently applied)."""
    return [16, 32, 4096, k.stream_grid * k.block * 16 + 4096 + 16]


def check_stream_copy(kern: Kernels, device, n_bytes: int) -> None:
    rng = np.random.default_rng(n_bytes)
    words = rng.integers(0, 2**32, size=n_bytes // 4, dtype=np.uint32)
    payloads = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0x80000000, 0x00000001], dtype=np.uint32)
    words[: payloads.size][: words.size] = payloads[: words.size]  # quiet and signalling NaNs with payloads, -0.0, a subnormal
    words[-payloads.size:] = payloads[-min(payloads.size, words.size):]
    guard = 4  # words: 16 bytes on each side keep the copy's base aligned
    src_host = np.concatenate([np.full(guard, 0x11111111, np.uint32), words, np.full(guard, 0x22222222, np.uint32)])
    src = torch.from_numpy(src_host.view(np.int32)).to(device)
    dst = torch.full((words.size + 2 * guard,), 0x33333333, dtype=torch.int32, device=device)
    kern.stream_copy(src[guard: guard + words.size].view(torch.float32), dst[guard: guard + words.size].view(torch.float32))
    got = dst.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got[guard: guard + words.size] != words)
    assert bad.size == 0, f"stream_copy: {n_bytes} bytes: words differ at {bad[:5]}"
    assert np.all(got[:guard] == 0x33333333) and np.all(got[guard + words.size:] == 0x33333333), f"stream_copy: {n_bytes} bytes: written outside dst"
    assert np.array_equal(src.cpu().numpy().view(np.uint32), src_host), f"stream_copy: {n_bytes} bytes: the source was modified"
