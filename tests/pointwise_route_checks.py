"""The checks that hold every launch form of ``atx_pointwise_stack`` (csrc/atx_pointwise.hip) to numpy's bits and name the form each
case is written for — plain functions over the callables under test and a device.  tests/test_gpu_pointwise_routes.py runs them on
``native.*`` on an MI355X; tests/test_pointwise_route_checks_catch_defects.py runs them on the CPU against a numpy stand-in that walks
the buffers as the kernels do, once as it is and once per planted defect.

A case is a small column or field stack, a program and the route it declares (``atx_last_route``: a diagnostic the dispatcher sets
immediately before its launch).  ``check_case`` asserts the route and then, with no element left out:

- every level whose stages are all plain COPY: the input's bit patterns (NaN payloads, signalling NaNs and -0.0 included);
- every arithmetic level: numpy's bits in the stack's own dtype (``native_double._apply_op``: one rounding per ufunc, the
  parameters rounded as ``np.float32(p)`` / ``np.float64(p)``); where numpy gives a NaN, a NaN.  float32 exactly as float64;
- an EXP / LOG level: the exact function (tests/exact_statements.py, 128-bit) of the argument as the stages before it leave it,
  within the budget tests/ulp_budgets.py derives for the operator (the one tests/test_gpu_ulp_budgets.py holds it to) — no number of its own here;
- out of place: the input allocation unchanged; everywhere: every element of the output allocation outside the levels — pitch
  padding beyond the 16-byte vector that holds the last level (column stacks; include/atx.h leaves the rest of that vector
  unspecified), all padding of field-major rows, the canary rows before and after — unchanged, bit for bit;
- in place: the bits of the out-of-place result.

Inputs carry quiet and signalling NaNs with payloads, +-0.0, +-inf, subnormals, the largest finite value and both neighbours of
every clip bound the programs use.  The mask's set bytes are 1, 2, 128 and 255; the bytes around it are set too, so a kernel
reading the byte of a neighbouring point past either end masks what numpy does not.

Shapes come from the kernels' own constants, read from the sources at import time: the launch's item count (vectors for the
no-loop kernels, chunks of kBlock * kPwUnroll vectors for the chunked ones, (kBlock / Cg) * kPwUnroll rows for the row-chunk kernel,
kBlock * U vectors of a field) sits on an exact multiple, one item past it, and at one item in all.
"""

from __future__ import annotations

import math
import os
import re
import zlib
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

# (the operators, the special values and the level-by-level comparison are shared with tests/gather_route_checks.py)
from level_program_checks import (AFF, ARITH, CLIP, CP, DIV, EXP, IMP, INV, LOG, MSK, MUL, SETNAN, TAFF, bits_type, compare_levels, first_difference, m, own, per_level,
                                  per_vector, pieces, poison_bits, reference, special_values, tname, vec_of)
from anemoi_transform_amd import native

COLUMNS, FIELDS = native.COLUMNS, native.FIELDS
ROUTES = ("sparse", "uniform", "runs", "table", "typed", "levels", "flat", "row_chunk", "row_chunk_scalar", "fields", "fields_scalar")
F32_LEVELS = (1, 3, 4, 5, 8, 9, 24, 25)  # every n_lev % VEC, and n_lev < VEC
F64_LEVELS = (1, 2, 3, 24, 25)


# ---- the kernels' constants ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Constants:
    block: int        # kBlock: lanes per workgroup
    unroll: int       # kPwUnroll: vectors a lane of the chunked kernels has in flight
    max_active: int   # kMaxActive: vector columns the sparse kernel takes
    max_uniform: int  # kMaxUniform: stages that travel by value
    max_runs: int     # kMaxRuns: runs per stage that travel by value
    max_stages: int   # kMaxStages: the C ABI's limit
    lds: int          # bytes of LDS a per-point kernel's tables may take
    stream_grid: int  # kStreamGrid: the workgroup cap of the grid-stride kernels

    def tall_levels(self) -> int:
        """2001 levels under the library's 64 KB: two float64 stages of per-level tables no longer fit (flat), three no per-vector table
        either (split program); scaled with the budget for the stand-in's small one."""
        return (2001 * self.lds // 65536) | 1


def read_constants() -> Constants:
    csrc = os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc")

    def find(name, pattern):
        with open(os.path.join(csrc, name)) as f:
            m = re.search(pattern, f.read())
        assert m, f"{name}: {pattern} not found"
        return int(m.group(1))

    return Constants(
        block=find("atx_common.hpp", r"constexpr int kBlock = (\d+);"),
        unroll=find("atx_pointwise.hip", r"constexpr int kPwUnroll = (\d+);"),
        max_active=find("atx_pointwise.hip", r"constexpr int kMaxActive = (\d+);"),
        max_uniform=find("atx_common.hpp", r"constexpr int kMaxUniform = (\d+);"),
        max_runs=find("atx_common.hpp", r"constexpr int kMaxRuns = (\d+);"),
        max_stages=find("atx_common.hpp", r"constexpr int kMaxStages = (\d+);"),
        lds=find("atx_pointwise.hip", r"lds_levels > (\d+) \* 1024") * 1024,
        stream_grid=find("atx_common.hpp", r"#define ATX_MAX_GRID (\d+)"),
    )


K = read_constants()


@dataclass
class Kernels:
    """The callables under test: ``native.pointwise_stack``, ``native.last_route`` and ``native.level_program`` (a program tensor
    with its ``host_prog`` / ``vec_prog`` companions)."""

    pointwise_stack: Callable
    last_route: Callable
    level_program: Callable


# ---- cases --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    route: str                      # the launch form the case is written for (out of place, or its only mode)
    np_dtype: type
    n_lev: int
    n_pts: int
    stages: tuple                   # stages[s][l] = (op, use_mask, p0, p1)
    layout: int = COLUMNS
    pitch: Optional[int] = None     # elements between rows; None: the vector-tight pitch (what Stack.empty allocates)
    y_pitch: Optional[int] = None   # the output's, out of place (None: the same)
    offset: int = 0                 # elements between the 16-byte aligned allocation and the base
    mask: Optional[int] = None      # None: no mask pointer; k: a mask view starting k bytes into its allocation
    modes: tuple = ("out", "in")
    route_in: Optional[str] = None  # in place, where the launch form differs
    strip: tuple = ()               # companions taken off the program: "host_prog", "vec_prog"; "vec_prog_off16": vec_prog 8 bytes off

    @property
    def vec(self) -> int:
        return 16 // np.dtype(self.np_dtype).itemsize

    @property
    def row_len(self) -> int:
        return self.n_lev if self.layout == COLUMNS else self.n_pts

    @property
    def n_rows(self) -> int:
        return self.n_pts if self.layout == COLUMNS else self.n_lev

    def tight(self) -> int:
        return -(-self.row_len // self.vec) * self.vec

    def x_pitch(self) -> int:
        return self.tight() if self.pitch is None else self.pitch

    def out_pitch(self) -> int:
        return self.x_pitch() if self.y_pitch is None else self.y_pitch

    def expected(self, mode: str) -> str:
        return self.route_in if (mode == "in" and self.route_in) else self.route


def points_for(slots: int, per_item: int) -> tuple:
    """Row counts that put ``n_pts * slots`` vectors on an exact multiple of ``per_item`` and one vector past a multiple."""
    exact = 2 * per_item // math.gcd(slots, per_item)
    past = pow(slots, -1, per_item) if slots % 2 and per_item > 1 else exact + 1
    if slots % 2 and per_item > 1 and past * slots < per_item:
        past += per_item
    return exact, past


def uniform_cases(k: Constants) -> list:
    out = []
    for dt, levels in ((np.float32, F32_LEVELS), (np.float64, F64_LEVELS)):
        v, t = vec_of(dt), tname(dt)
        for i, n_lev in enumerate(levels):
            C = -(-n_lev // v)
            exact, past = points_for(C, k.block)
            n_pts = (exact, past, 1)[i % 3] if C > 1 else (k.block, k.block + 1, 1)[i % 3]
            out.append(Case(f"uniform-1-stage-{t}-L{n_lev}-N{n_pts}", "uniform", dt, n_lev, n_pts, ((AFF,) * n_lev,)))
        for n_lev in (24, 25):
            C = -(-n_lev // v)
            exact, past = points_for(C, k.block)
            four = ((MUL,) * n_lev, (AFF,) * n_lev, (CLIP,) * n_lev, (IMP,) * n_lev)[: k.max_uniform]
            out.append(Case(f"uniform-{len(four)}-stages-{t}-L{n_lev}", "uniform", dt, n_lev, past, four))
            first, last = v, (C - 1) * v  # the split at vector column 1 and at C - 1 (n_lev = 25: the last vector is partial)
            two = (pieces(n_lev, (0, AFF), (first, MUL)), pieces(n_lev, (0, CLIP), (last, INV)))
            out.append(Case(f"uniform-two-pieces-{t}-L{n_lev}", "uniform", dt, n_lev, exact, two))
            for split, where in ((first, "col1"), (last, "last")):
                # sparse would take the few active columns of an in-place call: without vec_prog it cannot
                out.append(Case(f"uniform-first-piece-idle-{where}-{t}-L{n_lev}", "uniform", dt, n_lev, past,
                                (pieces(n_lev, (0, CP), (split, AFF)), pieces(n_lev, (0, CP), (split, DIV))), strip=("vec_prog",)))
                out.append(Case(f"uniform-second-piece-idle-{where}-{t}-L{n_lev}", "uniform", dt, n_lev, exact,
                                (pieces(n_lev, (0, INV), (split, CP)),), strip=("vec_prog",)))
            out.append(Case(f"uniform-mask-on-one-piece-{t}-L{n_lev}", "uniform", dt, n_lev, past,
                            (pieces(n_lev, (0, m(AFF)), (first, AFF)), pieces(n_lev, (0, CP), (last, MSK))), mask=0))
            for extra in (1, 3):
                out.append(Case(f"uniform-loose+{extra}-{t}-L{n_lev}", "uniform", dt, n_lev, points_for(C + extra, k.block)[extra // 2],
                                (pieces(n_lev, (0, m(MUL)), (last, CLIP)), (AFF,) * n_lev), pitch=(C + extra) * v, mask=0))
            out.append(Case(f"uniform-exp-log-{t}-L{n_lev}", "uniform", dt, n_lev, exact,
                            ((TAFF,) * n_lev, pieces(n_lev, (0, LOG), (first, CP)), pieces(n_lev, (0, CP), (last, EXP)))))
        # a split at a level that is no multiple of VEC: not by value
        off = (pieces(24, (0, AFF), (5, MUL)),)
        out.append(Case(f"uniform-declines-split-inside-a-vector-{t}", "levels", dt, 24, 7, off))
    out.append(Case("uniform-declines-split-inside-a-vector-2-stages-f32", "runs", np.float32, 24, 7,
                    (pieces(24, (0, AFF), (5, MUL)), (CLIP,) * 24)))
    return out


def runs_cases(k: Constants) -> list:
    dt, n_lev, v = np.float32, 25, 4
    C = -(-n_lev // v)
    exact, past = points_for(C, k.block)
    second = pieces(n_lev, (0, CLIP), (9, INV))
    two = pieces(n_lev, (0, AFF), (1, MUL))
    three = pieces(n_lev, (0, AFF), (1, MUL), (13, DIV))
    four = pieces(n_lev, (0, AFF), (1, MUL), (6, IMP), (n_lev - 1, DIV))[: n_lev]
    aba = pieces(n_lev, (0, AFF), (8, MUL), (17, AFF))
    near = (native.OP_AFFINE, 0, 1.5 + 2.0 ** -30, -3.0)  # another double, the same float32: ONE run with AFF
    assert np.float32(near[2]) == np.float32(AFF[2]) and near[2] != AFF[2]
    merged = pieces(n_lev, (0, MUL), (3, AFF), (7, near), (11, DIV), (22, IMP))  # five runs of doubles, four of floats
    five = pieces(n_lev, (0, MUL), (3, AFF), (7, INV), (11, DIV), (22, IMP))
    out = [
        Case("runs-2-f32", "runs", dt, n_lev, exact, (two, second)),
        Case("runs-3-f32", "runs", dt, n_lev, past, (three, second)),
        Case(f"runs-{k.max_runs}-f32", "runs", dt, n_lev, 1, (four, second, three)),
        Case("runs-a-b-a-f32", "runs", dt, n_lev, past, (aba, second)),
        Case("runs-merge-after-rounding-f32", "runs", dt, n_lev, exact, (merged, second)),
        Case("runs-fifth-run-declines-f32", "levels", dt, n_lev, exact, (five, second)),
        Case("runs-masked-run-f32", "runs", dt, n_lev, past, (pieces(n_lev, (0, AFF), (1, m(MUL)), (13, DIV)), second), mask=0),
        Case("runs-loose-f32", "runs", dt, n_lev, points_for(C + 1, k.block)[1], (three, pieces(n_lev, (0, CP), (2, m(CLIP)))), pitch=(C + 1) * v, mask=0),
        Case("runs-exp-log-f32", "runs", dt, n_lev, exact, ((TAFF,) * n_lev, pieces(n_lev, (0, LOG), (1, CP), (n_lev - 1, EXP)))),
        Case("runs-shape-in-f64-goes-to-levels", "levels", np.float64, n_lev, exact, (three, second)),
        Case("runs-shape-in-one-stage-goes-to-levels", "levels", dt, n_lev, exact, (three,)),
    ]
    return out


def table_cases(k: Constants) -> list:
    dt, v = np.float32, 4
    out = []
    for n_lev in (24, 25):
        C = -(-n_lev // v)
        exact, past = points_for(C, k.block)
        ops = per_vector(n_lev, v, (AFF, CLIP, CP, DIV, IMP, INV, MUL))
        out.append(Case(f"table-one-operator-per-vector-f32-L{n_lev}", "table", dt, n_lev, exact if n_lev == 24 else past, (ops,)))
    out.append(Case("table-one-vector-f32", "table", dt, 4, 1, (pieces(4, (0, MUL)),), strip=("host_prog",)))  # (with host_prog: uniform)
    out.append(Case("table-exp-log-f32", "table", dt, 24, 11, (per_vector(24, v, (TAFF, EXP, MUL, LOG, CLIP, DIV)),)))
    ops = per_vector(24, v, (AFF, CLIP, CP, DIV, IMP, INV))
    out.append(Case("table-declines-with-a-mask-pointer-f32", "levels", dt, 24, 7, (ops,), mask=0, route_in="typed"))
    mixed = ops[:9] + (MUL,) + ops[10:]
    out.append(Case("table-declines-a-mixed-vector-f32", "levels", dt, 24, 7, (mixed,)))
    return out


def typed_cases(k: Constants) -> list:
    out = []
    for n_lev in (24, 25):
        C = -(-n_lev // 2)
        exact, past = points_for(C, k.block)
        scale = tuple(own(MUL, l) for l in range(n_lev))
        out.append(Case(f"typed-scale-per-level-f64-L{n_lev}", "typed", np.float64, n_lev, exact if n_lev == 24 else past, (scale,)))
        out.append(Case(f"typed-scale-per-level-f32-L{n_lev}-in-place-only", "levels", np.float32, n_lev, 7, (scale,), route_in="typed"))
        out.append(Case(f"typed-code-0-untouched-f64-L{n_lev}", "typed", np.float64, n_lev, 9, ((CP, CP) + scale[2:],)))
        masked = tuple(own(m(AFF) if (l // 2) % 2 == 0 else INV, l) for l in range(n_lev))
        out.append(Case(f"typed-masked-and-unmasked-vectors-f64-L{n_lev}", "typed", np.float64, n_lev, 13, (masked,), mask=0))
    out.append(Case("typed-one-vector-f64", "typed", np.float64, 2, 1, ((own(MUL, 0), own(MUL, 1)),)))
    scale = tuple(own(MUL, l) for l in range(24))
    out.append(Case("typed-declines-float32-with-a-used-mask", "levels", np.float32, 24, 7, (tuple(m(e) for e in scale),), mask=0))
    out.append(Case("typed-float32-with-an-unused-mask-in-place", "levels", np.float32, 24, 7, (scale,), mask=0, route_in="typed"))
    out.append(Case("typed-declines-vec-prog-off-16-bytes-f64", "levels", np.float64, 24, 7, (scale,), strip=("vec_prog_off16",)))
    out.append(Case("typed-exp-log-f64", "typed", np.float64, 24, 11, (tuple(own(DIV, l) for l in range(20)) + (EXP, EXP, LOG, LOG),)))
    return out


def levels_cases(k: Constants) -> list:
    out = []
    chunk = k.block * k.unroll
    for dt, levels in ((np.float32, F32_LEVELS), (np.float64, F64_LEVELS)):
        v, t = vec_of(dt), tname(dt)
        for i, n_lev in enumerate(levels):
            C = -(-n_lev // v)
            exact, past = points_for(C, chunk)
            n_pts = (exact, past, 1)[i % 3] if C > 1 else (chunk, chunk + 1, 1)[i % 3]
            # (four levels or fewer are four runs or fewer: by value up to kMaxUniform stages)
            n_stage = (k.max_uniform + 1, k.max_stages)[i % 2] if n_lev <= k.max_runs else (2, 3, k.max_uniform + 1, k.max_stages)[i % 4]
            stages = tuple(per_level(n_lev, ARITH, shift=s) for s in range(n_stage))
            out.append(Case(f"levels-{n_stage}-stages-{t}-L{n_lev}-N{n_pts}", "levels", dt, n_lev, n_pts, stages))
        n_lev = 25
        masked = (per_level(n_lev, (AFF, m(MUL), CLIP, m(IMP), CP)), per_level(n_lev, (CP, m(INV), DIV)))
        out.append(Case(f"levels-mask-{t}", "levels", dt, n_lev, 37, masked, mask=0))
        idle = tuple(CP if (l // v) % 2 else e for l, e in enumerate(per_level(n_lev, (AFF, MUL, INV))))
        out.append(Case(f"levels-idle-vectors-{t}", "levels", dt, n_lev, 37, (idle, idle)))
        out.append(Case(f"levels-exp-log-{t}", "levels", dt, n_lev, 19, (per_level(n_lev, (TAFF,)), (CP, LOG, MUL, EXP) + per_level(n_lev - 4, ARITH))))
        out.append(Case(f"levels-uniform-program-of-{k.max_uniform + 1}-stages-{t}", "levels", dt, 24, 7,
                        tuple((e,) * 24 for e in (MUL, AFF, CLIP, IMP, INV, DIV)[: k.max_uniform + 1])))
        out.append(Case(f"levels-no-companions-{t}", "levels", dt, 9, 5, ((AFF,) * 9,), strip=("host_prog", "vec_prog")))
    n_lev = 2 * k.block + 3  # more vector columns than lanes
    out.append(Case("levels-more-columns-than-lanes-f64", "levels", np.float64, n_lev, 5, (per_level(n_lev, (AFF, MUL, INV)),)))
    return out


def flat_cases(k: Constants) -> list:
    n_lev, n_pts = k.tall_levels(), 37
    s0 = tuple((native.OP_AFFINE, 0, 1.0 + 0.001 * l, -0.25 * l) for l in range(n_lev))
    s1 = tuple((native.OP_CLIP, l % 2, 250.0, 300.0) if l % 3 else (native.OP_MUL, 0, 1.0 + 1.0 / (1 + l), 0.0) for l in range(n_lev))
    s2 = tuple(own(INV, l) for l in range(n_lev))
    s3 = tuple(own(DIV, l) if l % 2 else CP for l in range(n_lev))
    tr = (CP, EXP, LOG) + s3[3:]
    return [
        Case("flat-2-stages-f64", "flat", np.float64, n_lev, n_pts, (s0, s1), mask=0),
        Case("flat-2-stages-f32-fits-the-level-tables", "levels", np.float32, n_lev, n_pts, (s0, s1), mask=0),
        Case("flat-4-stages-f32", "flat", np.float32, n_lev, n_pts, (s0, s1, s2, s3), mask=0),
        Case("flat-split-program-3-stages-f64", "flat", np.float64, n_lev, n_pts, (s0, s1, s2), mask=0),
        Case("flat-exp-log-f64", "flat", np.float64, n_lev, 3, (tuple(own(TAFF, l) for l in range(n_lev)), tr)),
    ]


def sparse_cases(k: Constants) -> list:
    out = []
    A = k.max_active
    for dt in (np.float32, np.float64):
        v, t = vec_of(dt), tname(dt)

        def whole(C, cols, e=AFF, v=v):
            return tuple(e if l // v in cols else CP for l in range(C * v))

        other = "table" if dt == np.float32 else "typed"  # one stage, one kind per vector: where such a program goes out of place
        exact, past = points_for(1, k.block)
        out.append(Case(f"sparse-1-of-3-{t}", other, dt, 3 * v, k.block + 1, (whole(3, {1}),), route_in="sparse"))
        out.append(Case(f"sparse-1-of-2-declines-{t}", "uniform", dt, 2 * v, k.block + 1, (whole(2, {1}),)))
        cols = set(range(1, 3 * A, 3))
        out.append(Case(f"sparse-{A}-of-{3 * A}-{t}", other, dt, 3 * A * v, points_for(A, k.block)[0], (whole(3 * A, cols, MUL),), route_in="sparse"))
        cols = set(range(1, 3 * A + 3, 3))
        out.append(Case(f"sparse-{A + 1}-of-{3 * A + 3}-declines-{t}", other, dt, (3 * A + 3) * v, 3, (whole(3 * A + 3, cols, MUL),)))
        n_lev = 25
        last = tuple(own(DIV, l) if l == n_lev - 1 else CP for l in range(n_lev))
        out.append(Case(f"sparse-last-partial-vector-{t}", "uniform", dt, n_lev, 1, (last,), route_in="sparse"))
        C = -(-n_lev // v)
        two = (tuple(AFF if l in (5, n_lev - 1) else CP for l in range(n_lev)), tuple(m(CLIP) if l == 5 else (IMP if l == n_lev - 1 else CP) for l in range(n_lev)))
        out.append(Case(f"sparse-loose-masked-{t}", "runs" if dt == np.float32 else "row_chunk", dt, n_lev, points_for(2, k.block)[1], two, pitch=(C + 2) * v, mask=0, route_in="sparse"))
        out.append(Case(f"sparse-exp-log-{t}", "levels", dt, n_lev, 9, (tuple({4: EXP, 5: MUL, n_lev - 1: LOG}.get(l, CP) for l in range(n_lev)),), route_in="sparse"))
        out.append(Case(f"sparse-nothing-active-{t}", "none", dt, n_lev, 9, ((CP,) * n_lev, (CP,) * n_lev), modes=("in",)))
    return out


def row_chunk_cases(k: Constants) -> list:
    out = []
    for dt, levels in ((np.float32, F32_LEVELS), (np.float64, F64_LEVELS)):
        v, t = vec_of(dt), tname(dt)
        for i, n_lev in enumerate(levels):
            C = -(-n_lev // v)
            rows = (k.block // min(C, k.block)) * k.unroll  # rows a workgroup moves per iteration
            n_pts = (2 * rows, 2 * rows + 1, 1)[i % 3]
            stages = tuple(per_level(n_lev, ARITH, shift=s) for s in range(1 + i % 3))
            out.append(Case(f"row-chunk-unequal-pitches-{t}-L{n_lev}-N{n_pts}", "row_chunk", dt, n_lev, n_pts, stages, y_pitch=(C + 1) * v, modes=("out",)))
            rows = (k.block // min(n_lev, k.block)) * k.unroll
            n_pts = (2 * rows, 2 * rows + 1, 1)[(i + 1) % 3]
            if n_lev % v:  # a thin (or ragged) stack stored tight: no 16-byte vector holds a row's end
                out.append(Case(f"row-chunk-scalar-tight-{t}-L{n_lev}-N{n_pts}", "row_chunk_scalar", dt, n_lev, n_pts, stages, pitch=n_lev))
            out.append(Case(f"row-chunk-scalar-odd-pitch-{t}-L{n_lev}-N{n_pts}", "row_chunk_scalar", dt, n_lev, n_pts, stages, pitch=C * v + 1))
        if v > 2:  # two float32 levels stored tight (two float64 ones are a whole vector: below); the odd pitch: Cg = 2, kBlock / 2 rows per pass
            rows = (k.block // 2) * k.unroll
            stages = (per_level(2, (AFF, m(MUL))), per_level(2, (CLIP, INV)))
            out.append(Case(f"row-chunk-scalar-tight-{t}-L2-N{2 * rows}", "row_chunk_scalar", dt, 2, 2 * rows, stages, pitch=2, mask=0))
            out.append(Case(f"row-chunk-scalar-tight-{t}-L2-N1", "row_chunk_scalar", dt, 2, 1, stages, pitch=2, mask=1))
            out.append(Case(f"row-chunk-scalar-odd-pitch-{t}-L2-N{2 * rows + 1}", "row_chunk_scalar", dt, 2, 2 * rows + 1, stages, pitch=3, mask=0))
        out.append(Case(f"row-chunk-tight-two-levels-is-a-vector-{t}", "uniform", dt, v, 5, ((AFF,) * v,), pitch=v))
        n_lev = 25
        C = -(-n_lev // v)
        masked = (per_level(n_lev, (AFF, m(MUL), CLIP, CP)), tuple(CP if (l // v) % 2 else e for l, e in enumerate(per_level(n_lev, (m(INV), DIV)))))
        out.append(Case(f"row-chunk-base-off-16-bytes-{t}", "row_chunk_scalar", dt, n_lev, 37, masked, offset=1, mask=0))
        out.append(Case(f"row-chunk-loose-per-level-{t}", "row_chunk", dt, n_lev, 37, masked, pitch=(C + 1) * v, mask=0))
        out.append(Case(f"row-chunk-{k.max_stages}-stages-{t}", "row_chunk", dt, n_lev, 5, tuple(per_level(n_lev, ARITH, shift=s) for s in range(k.max_stages)), pitch=(C + 3) * v))
        tr = (per_level(n_lev, (TAFF,)), (CP, LOG, MUL, EXP) + per_level(n_lev - 4, ARITH))
        out.append(Case(f"row-chunk-exp-log-{t}", "row_chunk", dt, n_lev, 11, tr, pitch=(C + 1) * v))
        out.append(Case(f"row-chunk-scalar-exp-log-{t}", "row_chunk_scalar", dt, n_lev, 11, tr, pitch=n_lev))
    n_lev = 2 * k.block + 3  # more levels than lanes: a lane keeps three columns
    out.append(Case("row-chunk-scalar-more-levels-than-lanes-f64", "row_chunk_scalar", np.float64, n_lev, 2 * k.unroll + 1, (per_level(n_lev, (AFF, MUL, INV)),), pitch=n_lev))
    return out


def fields_cases(k: Constants) -> list:
    out = []
    for dt in (np.float32, np.float64):
        v, t = vec_of(dt), tname(dt)
        U = 1 if dt == np.float32 else 2  # fields_vectors_per_lane
        full = v * k.block * U
        sizes = [1, v - 1, v, v + 1, full - 1, full] + [full + r for r in range(1, v)] + [v * k.block * j + r for j in (1, 2) for r in (0, v)]
        n_lev = 4
        stages = (tuple(own(e, l) for l, e in enumerate((AFF, CP, m(CLIP), INV))), tuple(own(e, l) for l, e in enumerate((m(MUL), CP, IMP, CP))))
        for i, n_pts in enumerate(sorted(set(s for s in sizes if s >= 1))):
            out.append(Case(f"fields-{t}-N{n_pts}", "fields", dt, n_lev, n_pts, stages, layout=FIELDS, mask=0, pitch=-(-n_pts // v) * v + (v if i % 2 else 0)))
        for at in (1, 2, 3):
            out.append(Case(f"fields-mask-{at}-bytes-in-{t}", "fields", dt, n_lev, full + v + 1, stages, layout=FIELDS, mask=at))
        out.append(Case(f"fields-unused-mask-pointer-{t}", "fields", dt, 3, 2 * v + 1, ((AFF, CP, DIV),), layout=FIELDS, mask=1))
        n_pts = full + v + 1
        out.append(Case(f"fields-scalar-odd-pitch-{t}", "fields_scalar", dt, n_lev, n_pts, stages, layout=FIELDS, mask=3, pitch=n_pts + (1 if n_pts % 2 == 0 else 2)))
        out.append(Case(f"fields-scalar-base-off-16-bytes-{t}", "fields_scalar", dt, n_lev, n_pts, stages, layout=FIELDS, mask=0, offset=1))
        out.append(Case(f"fields-scalar-one-point-{t}", "fields_scalar", dt, 3, 1, ((AFF, CP, DIV),), layout=FIELDS, pitch=1))
        idle = (CP, AFF, CP, CP, m(MUL), CP)
        out.append(Case(f"fields-idle-between-active-{t}", "fields", dt, 6, 3 * v + 1, (idle, tuple(CP if e == CP else CLIP for e in idle)), layout=FIELDS, mask=0, pitch=4 * v + v))
        eight = tuple(tuple(own(ARITH[(s + l) % len(ARITH)], l) for l in range(3)) for s in range(k.max_stages))
        out.append(Case(f"fields-{k.max_stages}-stages-{t}", "fields", dt, 3, 2 * v + 1, eight, layout=FIELDS))
        out.append(Case(f"fields-scalar-{k.max_stages}-stages-{t}", "fields_scalar", dt, 3, 2 * v + 1, eight, layout=FIELDS, offset=1))
        tr = ((TAFF, TAFF, TAFF, CP), (MUL, EXP, LOG, SETNAN))
        out.append(Case(f"fields-exp-log-{t}", "fields", dt, 4, 3 * v + 1, tr, layout=FIELDS))
        out.append(Case(f"fields-scalar-exp-log-{t}", "fields_scalar", dt, 4, 3 * v + 1, tr, layout=FIELDS, pitch=3 * v + 3))
    return out


def all_cases(k: Constants = K) -> list:
    cases = (uniform_cases(k) + runs_cases(k) + table_cases(k) + typed_cases(k) + levels_cases(k) + flat_cases(k) + sparse_cases(k) +
             row_chunk_cases(k) + fields_cases(k))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


def declared_routes(cases) -> set:
    return {c.expected(mode) for c in cases for mode in c.modes} - {"none"}


# ---- inputs, reference ----------------------------------------------------------------------------------------------------------
def make_inputs(case: Case) -> np.ndarray:
    """[n_lev, n_pts]: values around 280, one in four around 0 (finite exponentials in float32), every third element a special one, in turn."""
    dt = case.np_dtype
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    x = (280.0 + 30.0 * rng.standard_normal((case.n_lev, case.n_pts))).astype(dt)
    small = rng.random(x.shape) < 0.25
    x[small] = (3.0 * rng.standard_normal(int(small.sum()))).astype(dt)
    flat = x.reshape(-1)
    sp = special_values(dt)
    at = np.arange(1 if flat.size > 1 else 0, flat.size, 3)
    shift = int(rng.integers(0, sp.size))
    flat.view(bits_type(dt))[at] = sp.view(bits_type(dt))[(np.arange(at.size) + shift) % sp.size]
    return x


def make_mask(case: Case) -> np.ndarray:
    """One byte per point: zero, or one of the set values 1, 2, 128, 255."""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()) + 1)
    set_ = rng.random(case.n_pts) < 0.4
    if case.n_pts > 1:
        set_[:2] = [True, False]
        set_[-1] = False  # (the byte after the last point is set)
    return np.where(set_, np.array([1, 2, 128, 255], dtype=np.uint8)[np.arange(case.n_pts) % 4], 0).astype(np.uint8)


# ---- storage --------------------------------------------------------------------------------------------------------------------
class Buffer:
    """``n_rows`` rows ``pitch`` apart, ``offset`` elements into a 16-byte aligned allocation, a canary row before and after.  Everything
    that is no level holds the poison pattern."""

    def __init__(self, case: Case, pitch: int, device, values: Optional[np.ndarray], fill: float = 12345.0):  # values None: an output
        dt, v = case.np_dtype, case.vec
        self.case, self.pitch = case, pitch
        guard = (-(-max(pitch, case.row_len) // v) + 1) * v
        self.base = guard + case.offset
        total = self.base + case.n_rows * pitch + guard
        host = poison_bits(dt, total, values is None).view(dt)
        rows = host[self.base: self.base + case.n_rows * pitch].reshape(case.n_rows, pitch)
        if values is None:
            rows[:, : case.row_len] = fill  # a finite value no result takes: an element never written shows
        else:
            rows[:, : case.row_len] = values.T if case.layout == COLUMNS else values
        self.before = host.view(bits_type(dt)).copy()
        self.backing = torch.from_numpy(host).to(device)
        assert self.backing.data_ptr() % 16 == 0
        self.view = self.backing[self.base:]
        assert (self.view.data_ptr() % 16 == 0) == (case.offset % v == 0)

    def bits(self) -> np.ndarray:
        return self.backing.cpu().numpy().view(bits_type(self.case.np_dtype))

    def split(self, bits: np.ndarray):
        """(levels [n_lev, n_pts], what the call may not touch: a boolean over the whole allocation)."""
        c = self.case
        rows = bits[self.base: self.base + c.n_rows * self.pitch].reshape(c.n_rows, self.pitch)
        levels = rows[:, : c.row_len].T if c.layout == COLUMNS else rows[:, : c.row_len]
        keep = np.ones(bits.size, dtype=bool)
        own_ = keep[self.base: self.base + c.n_rows * self.pitch].reshape(c.n_rows, self.pitch)
        # column stacks: the rest of the 16-byte vector that holds the last level is unspecified (include/atx.h), where the pitch has it
        own_[:, : min(c.tight(), self.pitch) if c.layout == COLUMNS else c.row_len] = False
        return levels.copy(), keep


class MaskBuffer:
    def __init__(self, case: Case, device):
        self.host = make_mask(case)
        alloc = np.full(case.mask + case.n_pts + 16, 255, dtype=np.uint8)  # set bytes all around
        alloc[case.mask: case.mask + case.n_pts] = self.host
        self.before = alloc.copy()
        self.backing = torch.from_numpy(alloc).to(device)
        assert self.backing.data_ptr() % 16 == 0
        self.view = self.backing[case.mask:]


def build_program(kern: Kernels, case: Case, device):
    prog = kern.level_program([list(st) for st in case.stages], device)
    for name in case.strip:
        if name == "host_prog":
            prog.host_prog = None
        elif name == "vec_prog":
            prog.vec_prog = {}
        else:
            assert name == "vec_prog_off16"
            moved = {}
            for tdt, table in prog.vec_prog.items():
                room = torch.zeros(table.numel() + 16, dtype=torch.uint8, device=table.device)
                assert room.data_ptr() % 16 == 0
                moved[tdt] = room[8: 8 + table.numel()]
                moved[tdt].copy_(table)
            prog.vec_prog = moved
    return prog


# ---- the check ------------------------------------------------------------------------------------------------------------------
def check_case(kern: Kernels, device, case: Case) -> dict:
    """Run the case in its modes; returns the routes taken."""
    dt = case.np_dtype
    uses_mask = any(e[1] for st in case.stages for e in st)
    assert case.mask is not None or not uses_mask, case.name
    x = make_inputs(case)
    mask = MaskBuffer(case, device) if case.mask is not None else None
    want, args = reference(x, case.stages, None if mask is None else mask.host)
    kw = dict(n_pts=case.n_pts, n_lev=case.n_lev, layout=case.layout, n_stage=len(case.stages), point_mask=None if mask is None else mask.view)
    taken, out_levels = {}, None
    for mode in case.modes:
        what = f"{case.name} [{'in place' if mode == 'in' else 'out of place'}]"
        prog = build_program(kern, case, device)
        if mode == "out":
            src = Buffer(case, case.x_pitch(), device, x)
            dst = Buffer(case, case.out_pitch(), device, None)
        else:
            src = dst = Buffer(case, case.x_pitch(), device, x)
        kern.pointwise_stack(src.view, dst.view, x_pitch=src.pitch, y_pitch=dst.pitch, prog=prog, **kw)
        taken[mode] = kern.last_route()
        assert taken[mode] == case.expected(mode), f"{what}: route {taken[mode]}, the case is written for {case.expected(mode)}"
        after = dst.bits()
        levels, keep = dst.split(after)
        compare_levels(case.np_dtype, case.stages, levels, x, want, args, what)
        moved = keep & (after != dst.before)
        if moved.any():
            at = int(np.flatnonzero(moved)[0]) - dst.base
            row, col = divmod(at, dst.pitch)
            where = f"row {row} element {col} (pitch {dst.pitch}, row length {case.row_len})" if 0 <= at < case.n_rows * dst.pitch else f"element {at} from the base"
            kind = "padding" if 0 <= at < case.n_rows * dst.pitch else "canary"
            raise AssertionError(f"{what}: {kind} written: {where} holds {int(after[at + dst.base]):#x}")
        if mode == "out":
            assert np.array_equal(src.bits(), src.before), f"{what}: the input was changed"
            out_levels = levels
        elif out_levels is not None:
            same = levels == out_levels
            assert same.all(), f"{what}: differs from the out-of-place result — {first_difference(levels.view(dt), out_levels.view(dt), ~same)}"
        if mask is not None:
            assert np.array_equal(mask.backing.cpu().numpy(), mask.before), f"{what}: the mask was written"
    return taken


def check_no_points(kern: Kernels, device) -> None:
    """A stack without points launches nothing: ``none``, after a call that did launch."""
    case = Case("one-point", "uniform", np.float32, 4, 1, ((AFF,) * 4,))
    check_case(kern, device, case)
    buf = Buffer(case, 4, device, make_inputs(case))
    prog = kern.level_program([list(st) for st in case.stages], device)
    kern.pointwise_stack(buf.view, buf.view, n_pts=0, n_lev=4, x_pitch=4, y_pitch=4, layout=COLUMNS, prog=prog, n_stage=1)
    assert kern.last_route() == "none", f"no points: route {kern.last_route()}"
    assert np.array_equal(buf.bits(), buf.before), "no points: the buffer was written"
