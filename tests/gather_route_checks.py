"""The checks that hold every launch form of the gather (csrc/atx_regrid.hip, atx_regrid_columns.inc, atx_regrid_fields.inc) to scipy's
and numpy's bits and name the form each case is written for — plain functions over the callables under test and a device.
tests/test_gpu_gather_routes.py runs them on ``native.*`` on an MI355X; tests/test_gather_route_checks_catch_defects.py runs them on
the CPU against a numpy stand-in that decides as the dispatcher does and walks the buffers as the kernels do, once as it is and once
per planted defect.

A case is a small source stack (or a batch of two), an index / weight table or a CSR matrix, perhaps a fused per-level program, and
the route it declares (``atx_last_gather_route``: a diagnostic the launchers fill immediately before the launch).  ``check_case``
asserts the route and then, with no element left out:

- a gather without a program: scipy's ``csr_matvec`` in the stack's own dtype (``oracle.csr_apply``), bit for bit in float32 as in
  float64 (where scipy has a NaN, a NaN); the unweighted k = 1 gather: a bit copy, NaN payloads, signalling NaNs and -0.0 included;
- program levels: the chain ``csr_matvec``, then numpy's statement stage by stage (tests/level_program_checks.py): arithmetic levels
  bit for bit in both widths, EXP / LOG levels against the exact function within the budget of tests/ulp_budgets.py;
- cases of one ``group`` run the same problem through different routes: the same bits, exp / log levels included;
- the output allocation starts as a canary pattern (a row nobody visited shows); the rows before and after the stack, the pitch
  padding beyond the 16-byte vector that holds the last level (column stacks) and all row padding (field-major stacks) stay untouched;
- sources, tables, ``tgt_rows`` and the mask are unchanged afterwards.

Sources carry quiet and signalling NaNs with payloads, +-0.0, +-inf, subnormals, the largest finite value and both neighbours of every
clip bound; weights include negative ones and exact zeros; padded rows include the all-absent row, the full one and a single entry in
the last slot, and absent entries carry a weight that must not be used.  The mask's set bytes are 1, 2, 128 and 255, the bytes
around it are set too, and in an ordered launch it is indexed by OUTPUT row while the tables are stored in visiting order.

Shapes come from the dispatcher's constants, read from the sources at import time, so that they stay on the boundaries when a
constant moves.  Cells an older test already holds to an oracle are not repeated: the plain gather at every compile-time and runtime
k, padded or not, direct and tiled, natural and ordered, one stack and two, both layouts — test_gpu_regrid_routes.py::
test_every_ladder_instantiation_gives_scipys_bits; the direct kernel's stripes past one group —
test_gpu_regrid_routes.py::test_direct_kernel_stripes_cover_every_row (one case here keeps the planted stripe defect honest).
"""

from __future__ import annotations

import functools
import os
import re
import zlib
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

from anemoi_transform_amd import native
from level_program_checks import (AFF, ARITH, CLIP, CLIP_HI, CLIP_LO, CP, DIV, EXP, IMP, INV, LOG, MSK, MUL, SETNAN, TAFF, bits_type, compare_levels, first_difference, m, own,
                                  per_level, pieces, poison_bits, reference, special_values, tname, vec_of)
from oracle import oracle
from pointwise_route_checks import points_for

COLUMNS, FIELDS = native.COLUMNS, native.FIELDS
N_SRC, N_TGT = 300, 131  # the base shape of tests/test_gpu_regrid_routes.py: two workgroups with a tail, no tile size divides 131
F32_LEVELS = (1, 3, 4, 5, 8, 9, 25)  # every n_lev % VEC, and n_lev < VEC
F64_LEVELS = (1, 2, 3, 25)
LADDER = (1, 2, 3, 4, 5, 6, 7, 8, 12, 16)  # the compile-time k of the column ladder (dispatch_cols_ell); the field ladder stops at 4


# ---- the dispatcher's constants -------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Constants:
    block: int               # kBlock: lanes per workgroup of the CSR and field-major kernels
    ell_block: int           # kEllBlock: lanes per workgroup of the fixed-k column kernels
    xcds: int                # kXcds
    max_batch: int           # kMaxBatch: stacks per launch
    long_row_stripe: int     # kLongRowStripe
    csr_stripe: int          # kCsrStripe
    csr_stripe_min_mean: float
    max_uniform: int
    max_runs: int
    max_table: int
    max_stages: int
    fields_chunk: int        # kFieldsChunk
    lds_rows: int            # bytes the tiled kernel's index / weight rows may take (48 KB)
    lds_max: int             # bytes of LDS a gather launch may ask for (64 KB)
    head4_mean: float        # fields_csr: mean row length up to which the head kernel keeps 4 entries in registers
    head8_mean: float        # ... 8 entries; beyond: the long-row kernel
    tile_items: tuple        # pick_tile: (target, vector) items per workgroup without / with an epilogue
    csr_cap: int             # launch_cols_csr: entries of a tile staged in LDS at the most


def read_constants() -> Constants:
    csrc = os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc")

    def find(name, pattern, kind=int, group=1):
        with open(os.path.join(csrc, name)) as f:
            found = re.search(pattern, f.read())
        assert found, f"{name}: {pattern} not found"
        return kind(found.group(group))

    cols, fields, common, decl = "atx_regrid_columns.inc", "atx_regrid_fields.inc", "atx_common.hpp", "atx_regrid_decl.hpp"
    return Constants(
        block=find(common, r"constexpr int kBlock = (\d+);"),
        ell_block=find(cols, r"constexpr int kEllBlock = (\d+);"),
        xcds=find(common, r"constexpr int kXcds = (\d+);"),
        max_batch=find(decl, r"constexpr int kMaxBatch = (\d+);"),
        long_row_stripe=find(cols, r"constexpr unsigned kLongRowStripe = (\d+);"),
        csr_stripe=find(cols, r"constexpr int kCsrStripe = (\d+);"),
        csr_stripe_min_mean=find(cols, r"constexpr double kCsrStripeMinMean = ([\d.]+);", float),
        max_uniform=find(common, r"constexpr int kMaxUniform = (\d+);"),
        max_runs=find(common, r"constexpr int kMaxRuns = (\d+);"),
        max_table=find(cols, r"constexpr int kMaxTable = (\d+);"),
        max_stages=find(common, r"constexpr int kMaxStages = (\d+);"),
        fields_chunk=find(fields, r"constexpr int kFieldsChunk = (\d+);"),
        lds_rows=find(cols, r"row_bytes > (\d+) \* 1024\) tile =") * 1024,
        lds_max=find(cols, r"if \(prog && lds > (\d+) \* 1024\) return ATX_SPLIT_PROGRAM") * 1024,
        head4_mean=find(fields, r"with_flag\(mean <= ([\d.]+),", float),
        head8_mean=find(fields, r"if \(mean <= ([\d.]+)\) \{  // short rows", float),
        tile_items=(find(decl, r"const int items = epilogue \? (\d+) : (\d+);", int, 2), find(decl, r"const int items = epilogue \? (\d+) : (\d+);")),
        csr_cap=find(cols, r"if \(cap > (\d+)\) cap = "),
    )


K = read_constants()

# The first four fields of every name the launchers can produce (include/atx.h: atx_last_gather_route) — a new launch form without a
# case written for it fails test_every_route_has_a_case.  "split" stands where the epilogue did not fit and the plain gather ran.
ROUTE_CLASSES = tuple(
    [f"cols_ell/direct/{e}/{w}" for e in ("none", "uniform", "runs") for w in ("vec", "scalar")] + ["cols_ell/direct/table/vec"] +
    [f"cols_ell/tiled/{e}/{w}" for e in ("none", "lds") for w in ("vec", "scalar")] + ["cols_ell/direct/split/vec", "cols_ell/tiled/split/vec"] +
    [f"cols_csr/tiled/{e}/{w}" for e in ("none", "lds") for w in ("vec", "scalar")] + ["cols_csr/tiled/split/vec"] +
    [f"fields_ell/lanes/{e}/lane" for e in ("none", "global")] +
    [f"fields_csr/{kern}/{e}/lane" for kern in ("head4", "head8", "long") for e in ("none", "global")])


def route_class(route: str) -> str:
    return "/".join(route.split("/")[:4])


def ladder_k(k: int, padded: bool, limit: int = 16) -> int:
    """The compile-time k the ladders instantiate for ``k`` (0: the runtime loop); padded tables start at 3."""
    return k if (k in LADDER and k <= limit and k >= (3 if padded else 1)) else 0


@dataclass
class Kernels:
    """The callables under test, ``native.*`` of the same names."""

    regrid_ell: Callable
    regrid_ell_batch: Callable
    regrid_csr: Callable
    last_gather_route: Callable
    last_route: Callable
    level_program: Callable
    set_tuning: Callable


# ---- cases --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    route: str                        # the launch form the case is written for (atx_last_gather_route)
    np_dtype: type
    table: str = "ell"                # "ell": index / weight rows of k entries; "csr": rows of ``lengths``
    layout: int = COLUMNS
    n_lev: int = 5
    n_tgt: int = N_TGT
    n_src: int = N_SRC
    k: int = 4
    padded: bool = False
    weighted: bool = True
    ordered: bool = False             # tables stored in a visiting order, tgt_rows given
    n_stack: int = 1
    stages: Optional[tuple] = None    # stages[s][l] = (op, use_mask, p0, p1)
    mask: Optional[int] = None        # None: no mask pointer; b: a mask view starting b bytes into its allocation (b >= 1: a set byte before it)
    src_pitch: Optional[int] = None   # elements between rows; None: the vector-tight pitch (field-major: one vector of padding more)
    out_pitch: Optional[int] = None
    offset: int = 0                   # elements between the 16-byte aligned allocation and the base of every OUTPUT
    tile: int = 0                     # set_tuning
    strip: tuple = ()                 # companions taken off the program: "host_prog", "vec_prog"
    lengths: Optional[tuple] = None   # csr: entries of every row
    pw_route: Optional[str] = None    # split: the per-point form that finishes the program (atx_last_route)
    group: Optional[str] = None       # cases of one group share the problem: the same bits on every route

    @property
    def vec(self) -> int:
        return 16 // np.dtype(self.np_dtype).itemsize

    def tight(self, n_pts: int) -> int:
        row = self.n_lev if self.layout == COLUMNS else n_pts
        return -(-row // self.vec) * self.vec + (self.vec if self.layout == FIELDS else 0)

    def sp(self) -> int:
        return self.tight(self.n_src) if self.src_pitch is None else self.src_pitch

    def op(self) -> int:
        return self.tight(self.n_tgt) if self.out_pitch is None else self.out_pitch

    def problem_key(self) -> tuple:
        return (self.group or self.name, self.np_dtype, self.table, self.n_lev, self.n_tgt, self.n_src, self.k, self.padded, self.weighted, self.n_stack,
                self.stages, self.mask is not None, self.lengths)


def route_name(table, kernel, epilogue, width, k=0, padded=False, weighted=True, stripe=False, ordered=False) -> str:
    return "/".join([table, kernel, epilogue, width, f"k{k}", "padded" if padded else "plain", "weighted" if weighted else "pure",
                     "stripe" if stripe else "range", "ordered" if ordered else "natural"])


def direct(epilogue, k, *, c: Constants = K, width="vec", padded=False, weighted=True, ordered=False) -> str:
    """The direct kernel's name: rows of 5 entries and more in natural order have their workgroups dealt in stripes."""
    return route_name("cols_ell", "direct", epilogue, width, k, padded, weighted, k >= 5 and not ordered, ordered)


def tiled(epilogue, k, *, width="vec", padded=False, weighted=True, ordered=False) -> str:
    """The tiled kernel's: k > 4 and every k outside the ladder run its runtime loop."""
    kt = ladder_k(k, padded, limit=4) if weighted else 1
    return route_name("cols_ell", "tiled", epilogue, width, kt, padded, weighted, False, ordered)


# programs over n_lev levels -----------------------------------------------------------------------------------------------------
def uniform_programs(n_lev: int, v: int, c: Constants) -> dict:
    """name -> (stages, uses the mask, the epilogue that serves it on the direct kernel); the split of two pieces on the last vector boundary."""
    split = max(v, (n_lev - 1) // v * v) if n_lev > v else None
    two = (lambda a, b: pieces(n_lev, (0, a), (split, b))) if split else (lambda a, b: (a,) * n_lev)
    four = ((MUL,) * n_lev, two(AFF, INV), (CLIP,) * n_lev, (m(IMP),) * n_lev, (DIV,) * n_lev, (CLIP_LO,) * n_lev, (AFF,) * n_lev, (CLIP_HI,) * n_lev)
    return {
        "one-piece": (((AFF,) * n_lev,), False, "uniform"),
        "two-pieces": ((two(m(MUL), CLIP),), True, "uniform"),
        "two-stages": (((AFF,) * n_lev, two(CLIP, INV)), False, "uniform"),
        f"{c.max_uniform}-stages": (four[: c.max_uniform], True, "uniform"),
        f"{c.max_uniform + 1}-stages-leave": (four[: c.max_uniform + 1], True, "lds"),
        "exp-log": (((TAFF,) * n_lev, two(LOG, EXP)), False, "uniform"),
        "set-nan-masked-copy": ((two(SETNAN, MSK), (m(DIV),) * n_lev), True, "uniform"),
    }


def runs_programs(n_lev: int, c: Constants) -> dict:
    """Runs with boundaries inside 16-byte vectors (n_lev >= 9)."""
    assert n_lev >= 9 and c.max_runs == 4
    four = pieces(n_lev, (0, AFF), (1, MUL), (3, IMP), (6, DIV))
    second = pieces(n_lev, (0, CLIP), (5, INV))
    five = pieces(n_lev, (0, AFF), (1, DIV), (3, IMP), (6, INV), (7, CLIP))
    five_madd = pieces(n_lev, (0, AFF), (1, MUL), (3, CP), (6, own(AFF, 1)), (7, own(MUL, 2)))
    return {
        f"{c.max_runs}-runs": ((four, second), False, "runs"),
        "masked-run": ((pieces(n_lev, (0, AFF), (1, m(MUL)), (6, CLIP_HI)), pieces(n_lev, (0, CP), (2, m(CLIP_LO)))), True, "runs"),
        "one-stage": ((pieces(n_lev, (0, INV), (3, DIV), (7, CP)),), False, "runs"),
        "exp-log": (((TAFF,) * n_lev, pieces(n_lev, (0, LOG), (1, CP), (n_lev - 2, EXP))), False, "runs"),
        "fifth-run-leaves": ((five, second), False, "lds"),
        "fifth-run-of-multiply-adds-takes-the-table": ((five_madd,), False, "table"),
    }


def table_programs(n_lev: int, c: Constants) -> dict:
    """The multiply-add family with more than kMaxRuns runs in a stage: only the per-vector table takes them to the direct kernel."""
    assert n_lev >= 9
    madd = (AFF, MUL, CP)
    own_params = per_level(n_lev, madd)  # every level parameters of its own: n_lev runs, every vector mixed
    some_masked = tuple(m(e) if l % 3 == 1 else e for l, e in enumerate(per_level(n_lev, madd, shift=1)))
    stages4 = tuple(per_level(n_lev, madd, shift=s) for s in range(c.max_table))
    return {
        "per-level-parameters": ((own_params,), False, "table"),
        "mask-on-some-levels": ((own_params, some_masked), True, "table"),
        f"{c.max_table}-stages": (stages4, False, "table"),
        f"{c.max_table + 1}-stages-leave": (stages4 + (per_level(n_lev, madd, shift=7),), False, "lds"),
        "a-clip-among-them-leaves": ((own_params, tuple(CLIP if l == 4 else e for l, e in enumerate(own_params))), False, "lds"),
    }


def general_programs(n_lev: int, c: Constants) -> dict:
    """What only the tiled kernel's LDS tables serve: general operators level by level, kMaxUniform + 1 to kMaxStages stages."""
    out = {}
    for n_stage in range(c.max_uniform + 1, c.max_stages + 1):
        stages = tuple(per_level(n_lev, ARITH, shift=s) for s in range(n_stage))
        if n_stage % 2:  # the mask on some levels of some stages
            stages = tuple(tuple(m(e) if (l + s) % 4 == 0 else e for l, e in enumerate(st)) for s, st in enumerate(stages))
        out[f"{n_stage}-stages"] = (stages, bool(n_stage % 2), "lds")
    if n_lev >= 4:
        out["exp-log"] = ((per_level(n_lev, (TAFF,)), (CP, LOG, MUL, EXP) + per_level(n_lev - 4, ARITH)) + tuple(((CP,) * 4 + per_level(n_lev - 4, ARITH, shift=s)) for s in range(c.max_uniform - 1)), False, "lds")
    return out


def with_program(name, route, dt, prog, **kw) -> Case:
    stages, masked, _ = prog
    return Case(name, route, dt, stages=stages, mask=1 if masked else None, **kw)


def direct_epilogue_cases(c: Constants) -> list:
    """cols_ell direct with the uniform, runs and table epilogues: every program at k = 4, one program of each at every k of the ladder's
    edges — 1 weighted and pure, 4, 5, 8, 12, 16, padded 3 and 8 — striped (natural order) and in ranges (ordered), one stack and two."""
    out = []
    n_lev = 9
    for dt in (np.float32, np.float64):
        t, v = tname(dt), vec_of(dt)
        families = {"uniform": uniform_programs(n_lev, v, c), "runs": runs_programs(n_lev, c), "table": table_programs(n_lev, c)}
        for family, programs in families.items():
            for pname, prog in programs.items():
                epi = prog[2]
                route = direct(epi, 4) if epi != "lds" else tiled("lds", 4)
                for strip, served in (((), route), (("host_prog",), tiled("lds", 4))):  # without host_prog nothing reaches the direct kernel
                    if strip and served == route:
                        continue
                    out.append(with_program(f"direct-{family}-{pname}-{t}-k4" + ("-no-host-prog" if strip else ""), served, dt, prog, n_lev=n_lev, k=4, strip=strip,
                                            group=f"k4-{family}-{pname}-{t}"))
            main = {"uniform": "two-pieces", "runs": "masked-run", "table": "mask-on-some-levels"}[family]
            prog = programs[main]
            variants = [(1, False, True), (1, False, False), (4, False, True), (5, False, True), (8, False, True), (12, False, True), (16, False, True), (3, True, True), (8, True, True)]
            for i, (k, padded, weighted) in enumerate(variants):
                tag = f"k{k}" + ("-padded" if padded else "") + ("" if weighted else "-pure")
                for ordered in ((False, True) if (k >= 5 or i % 2) else (False,)):
                    n_stack = 2 if (i + ordered) % 2 else 1
                    out.append(with_program(f"direct-{family}-{t}-{tag}" + ("-ordered" if ordered else "") + (f"-batch{n_stack}" if n_stack > 1 else ""),
                                            direct(family, k, padded=padded, weighted=weighted, ordered=ordered), dt, prog, n_lev=n_lev, k=k, padded=padded,
                                            weighted=weighted, ordered=ordered, n_stack=n_stack))
        # the table route needs its companions: no vec_prog, no table
        prog = families["table"]["per-level-parameters"]
        out.append(with_program(f"direct-table-without-vec-prog-leaves-{t}", tiled("lds", 4), dt, prog, n_lev=n_lev, k=4, strip=("vec_prog",), group=f"k4-table-per-level-parameters-{t}"))
    return out


def shape_cases(c: Constants) -> list:
    """The launch at one item, n_tgt * C on an exact multiple of kEllBlock and one item past it, n_lev over every remainder of the vector
    width — with a uniform program of two pieces and the mask, and as the plain and the pure gather."""
    out = []
    for dt, levels in ((np.float32, F32_LEVELS), (np.float64, F64_LEVELS)):
        t, v = tname(dt), vec_of(dt)
        for i, n_lev in enumerate(levels):
            C = -(-n_lev // v)
            exact, past = points_for(C, c.ell_block)
            n_tgt = ((exact, past, 1)[i % 3]) if C > 1 else (c.ell_block, c.ell_block + 1, 1)[i % 3]
            prog = uniform_programs(n_lev, v, c)["two-pieces" if n_lev > v else "one-piece"]
            kk = (4, 1, 5)[i % 3]
            out.append(with_program(f"shape-uniform-{t}-L{n_lev}-N{n_tgt}-k{kk}", direct("uniform", kk), dt, prog, n_lev=n_lev, n_tgt=n_tgt, k=kk))
            out.append(Case(f"shape-pure-{t}-L{n_lev}-N{n_tgt}", direct("none", 1, weighted=False), dt, n_lev=n_lev, n_tgt=n_tgt, k=1, weighted=False))
            out.append(Case(f"shape-plain-{t}-L{n_lev}-N{n_tgt}-tiled", tiled("none", 4), dt, n_lev=n_lev, n_tgt=n_tgt, k=4, tile=8))
        for n_tgt in (1, c.ell_block, c.ell_block + 1):  # one vector per target: items = targets
            out.append(Case(f"shape-plain-{t}-one-vector-N{n_tgt}", direct("none", 4), dt, n_lev=v, n_tgt=n_tgt, k=4))
        # weighted k = 1 (the ladder's `case 1`, not the pure gather): 0 + w * x, scipy's -0.0 -> +0.0 and quieted NaNs
        out.append(Case(f"shape-plain-{t}-k1-weighted", direct("none", 1), dt, n_lev=5, k=1))
    # one case past a whole group of stripes (kXcds x kLongRowStripe workgroups): the permutation visits every workgroup once
    n_tgt = (c.xcds * c.long_row_stripe + 1) * c.ell_block + 7
    out.append(Case("shape-plain-f32-stripes-past-one-group", direct("none", 5, width="scalar"), np.float32, n_lev=1, n_tgt=n_tgt, k=5, src_pitch=1, out_pitch=1))
    return out


def tiled_cases(c: Constants) -> list:
    """cols_ell tiled with the lds epilogue: runtime k 9 and 17, plain and padded; a forced tile at K <= 4; general operators at
    kMaxUniform + 1 to kMaxStages stages; k = 64 on a 3-level stack (the 48 KB clamp of the tile's rows), with and without a program."""
    out = []
    for dt in (np.float32, np.float64):
        t, v = tname(dt), vec_of(dt)
        n_lev = 9
        general = general_programs(n_lev, c)
        for pname, prog in general.items():
            out.append(with_program(f"tiled-general-{pname}-{t}-k4", tiled("lds", 4), dt, prog, n_lev=n_lev, k=4))
        five = general[f"{c.max_uniform + 1}-stages"]
        for i, (k, padded) in enumerate(((9, False), (9, True), (17, False), (17, True), (2, True))):  # (padded 2: below the padded ladder)
            tag = f"k{k}" + ("-padded" if padded else "")
            ordered, n_stack = bool(i % 2), 1 + (i // 2) % 2
            out.append(with_program(f"tiled-general-{t}-{tag}" + ("-ordered" if ordered else "") + (f"-batch{n_stack}" if n_stack > 1 else ""),
                                    tiled("lds", k, padded=padded, ordered=ordered), dt, five, n_lev=n_lev, k=k, padded=padded, ordered=ordered, n_stack=n_stack))
        uni = uniform_programs(n_lev, v, c)["two-pieces"]
        for k, padded, weighted in ((1, False, False), (1, False, True), (3, True, True), (4, False, True), (8, False, True)):  # a forced tile: eligible programs through LDS
            tag = f"k{k}" + ("-padded" if padded else "") + ("" if weighted else "-pure")
            out.append(with_program(f"tiled-forced-tile-uniform-{t}-{tag}", tiled("lds", k, padded=padded, weighted=weighted), dt, uni, n_lev=n_lev, k=k, padded=padded,
                                    weighted=weighted, tile=8, group=f"k4-uniform-two-pieces-{t}" if (k, padded) == (4, False) else None))
        # k = 64 over 3 levels: pick_tile asks for more targets than 48 KB of rows hold
        row_bytes = 64 * (4 + np.dtype(dt).itemsize)
        assert min(256, N_TGT) * row_bytes > c.lds_rows
        out.append(Case(f"tiled-k64-rows-clamped-{t}", tiled("none", 64), dt, n_lev=3, k=64))
        out.append(with_program(f"tiled-k64-rows-clamped-{t}-program", tiled("lds", 64), dt, uniform_programs(3, v, c)["two-stages"], n_lev=3, k=64))
    return out


def scalar_cases(c: Constants) -> list:
    """VEC = 1 with a program: an odd pitch, a base off the 16-byte boundary, a tight one-level stack — direct (uniform, runs), tiled, CSR."""
    out = []
    for dt in (np.float32, np.float64):
        t, v = tname(dt), vec_of(dt)
        n_lev = 9
        uni, runs = uniform_programs(n_lev, 1, c), runs_programs(n_lev, c)
        table = table_programs(n_lev, c)["mask-on-some-levels"]
        odd = dict(n_lev=n_lev, src_pitch=n_lev + 2, out_pitch=n_lev)  # 11 and 9 elements: no multiple of a vector
        off = dict(n_lev=n_lev, offset=1)
        for how, kw in (("odd-pitch", odd), ("base-off-16-bytes", off)):
            # (with VEC = 1 any level is a vector boundary: a split anywhere travels by value)
            out.append(with_program(f"scalar-{how}-uniform-{t}", direct("uniform", 4, width="scalar"), dt, ((pieces(n_lev, (0, m(MUL)), (5, CLIP)),), True, "uniform"), k=4, **kw))
            out.append(with_program(f"scalar-{how}-runs-{t}", direct("runs", 4, width="scalar"), dt, runs["masked-run"], k=4, **kw))
            out.append(with_program(f"scalar-{how}-table-eligible-takes-lds-{t}", tiled("lds", 4, width="scalar"), dt, table, k=4, **kw))
            out.append(with_program(f"scalar-{how}-tiled-k9-{t}", tiled("lds", 9, width="scalar"), dt, general_programs(n_lev, c)[f"{c.max_uniform + 1}-stages"], k=9, **kw))
            out.append(Case(f"scalar-{how}-plain-{t}", direct("none", 4, width="scalar"), dt, k=4, **kw))
            out.append(Case(f"scalar-{how}-plain-tiled-k9-{t}", tiled("none", 9, width="scalar"), dt, k=9, **kw))
            lengths = csr_lengths(N_TGT, 3, seed=5)
            out.append(with_program(f"scalar-{how}-csr-{t}", route_name("cols_csr", "tiled", "lds", "scalar"), dt, uni["two-stages"], table="csr", lengths=lengths, **kw))
            out.append(Case(f"scalar-{how}-csr-plain-{t}", route_name("cols_csr", "tiled", "none", "scalar"), dt, table="csr", lengths=lengths, **kw))
        one = dict(n_lev=1, src_pitch=1, out_pitch=1)
        out.append(with_program(f"scalar-one-level-uniform-{t}", direct("uniform", 4, width="scalar"), dt, (((m(AFF),), (CLIP,)), True, "uniform"), k=4, **one))
        out.append(with_program(f"scalar-one-level-uniform-{t}-k8-ordered", direct("uniform", 8, width="scalar", ordered=True), dt, (((m(AFF),), (CLIP,)), True, "uniform"), k=8, ordered=True, **one))
        out.append(with_program(f"scalar-one-level-tiled-{t}", tiled("lds", 4, width="scalar"), dt, (((m(AFF),), (CLIP,)), True, "lds"), k=4, tile=8, **one))
        out.append(with_program(f"scalar-one-level-csr-{t}", route_name("cols_csr", "tiled", "lds", "scalar"), dt, (((m(AFF),), (CLIP,)), True, "lds"), table="csr",
                                lengths=csr_lengths(N_TGT, 3, seed=6), **one))
    return out


def loose_pitch_cases(c: Constants) -> list:
    """Pitches with room beyond the 16-byte vector that holds the last level: one vector and three more on the output, another count on
    the source — on every column kernel and epilogue, vector-wide and scalar.  The padding holds the poison pattern and must keep it."""
    out = []
    n_lev = 9
    for dt in (np.float32, np.float64):
        t, v = tname(dt), vec_of(dt)
        tight = -(-n_lev // v) * v
        uni, runs, table = uniform_programs(n_lev, v, c), runs_programs(n_lev, c), table_programs(n_lev, c)
        general = general_programs(n_lev, c)[f"{c.max_uniform + 1}-stages"]
        lengths = csr_lengths(N_TGT, 3, seed=9)
        for extra, src_extra in ((1, 2), (3, 0)):
            kw = dict(n_lev=n_lev, out_pitch=tight + extra * v, src_pitch=tight + src_extra * v)
            tag = f"{t}-out+{extra}-src+{src_extra}"
            out.append(with_program(f"loose-uniform-{tag}", direct("uniform", 4), dt, uni["two-pieces"], k=4, **kw))
            out.append(with_program(f"loose-runs-{tag}-k8-ordered", direct("runs", 8, ordered=True), dt, runs["masked-run"], k=8, ordered=True, **kw))
            out.append(with_program(f"loose-table-{tag}-k3-padded-batch2", direct("table", 3, padded=True), dt, table["mask-on-some-levels"], k=3, padded=True, n_stack=2, **kw))
            out.append(Case(f"loose-pure-{tag}", direct("none", 1, weighted=False), dt, k=1, weighted=False, **kw))
            out.append(with_program(f"loose-tiled-{tag}-k9", tiled("lds", 9), dt, general, k=9, **kw))
            out.append(with_program(f"loose-csr-{tag}", route_name("cols_csr", "tiled", "lds", "vec"), dt, general, table="csr", lengths=lengths, **kw))
            odd = dict(n_lev=n_lev, out_pitch=n_lev + 2 * extra, src_pitch=n_lev + 2 * src_extra)  # odd element counts: the scalar width, with padding
            out.append(with_program(f"loose-scalar-uniform-{tag}", direct("uniform", 4, width="scalar"), dt, uni["two-stages"], k=4, **odd))
            out.append(with_program(f"loose-scalar-tiled-{tag}-k9", tiled("lds", 9, width="scalar"), dt, general, k=9, **odd))
            out.append(with_program(f"loose-scalar-csr-{tag}", route_name("cols_csr", "tiled", "lds", "scalar"), dt, general, table="csr", lengths=lengths, **odd))
    return out


# ---- the dispatcher's decisions, restated (tests/native_double.py names its route with them, the stand-in of
# tests/test_gather_route_checks_catch_defects.py launches what they say; the device is the judge of both) ------------------------------
def tables_bytes(n_stage: int, C: int, vec: int, size: int) -> int:
    """atx_common.hpp: level_tables_lds_bytes."""
    return (n_stage * C * vec * (2 * size + 1) + 15) & ~15


def pick_tile(n_tgt: int, C: int, epilogue: bool, c: Constants) -> int:
    """atx_regrid_decl.hpp: pick_tile."""
    tile = (c.tile_items[1 if epilogue else 0] // C + 2) // 4 * 4
    return min(max(tile, 8), 256, n_tgt)


def same_op(T, a, b) -> bool:
    """Two entries of a program are one operator: op, use_mask, and the parameters as the kernel sees them (rounded to the stack's type)."""
    return (int(a["op"]) == int(b["op"]) and (int(a["use_mask"]) != 0) == (int(b["use_mask"]) != 0) and
            T(a["p0"]).tobytes() == T(b["p0"]).tobytes() and T(a["p1"]).tobytes() == T(b["p1"]).tobytes())


def uniform_form(T, P, have_mask: bool, n_lev: int, vec: int, c: Constants):
    """atx_common.hpp: uniform_level_program — per stage (first vector column of the second piece, first piece, second piece), or None."""
    if not 1 <= P.shape[0] <= c.max_uniform:
        return None
    C = -(-n_lev // vec)
    out = []
    for row in P:
        l = 1
        while l < n_lev and same_op(T, row[l], row[0]):
            l += 1
        if l == n_lev:
            out.append((C, row[0], row[0]))
            continue
        if l % vec or any(not same_op(T, row[j], row[l]) for j in range(l + 1, n_lev)):
            return None
        out.append((l // vec, row[0], row[l]))
    if any((int(a["use_mask"]) or int(b["use_mask"])) and not have_mask for _, a, b in out):
        return None
    return out


def runs_form(T, P, have_mask: bool, n_lev: int, c: Constants):
    """atx_common.hpp: runs_level_program — per stage [(first level, operator)], or None."""
    if not 1 <= P.shape[0] <= c.max_uniform:
        return None
    out = []
    for row in P:
        runs = []
        for l in range(n_lev):
            if runs and same_op(T, row[l], runs[-1][1]):
                continue
            if len(runs) == c.max_runs:
                return None
            runs.append((l, row[l]))
        if any(int(e["use_mask"]) and not have_mask for _, e in runs):
            return None
        out.append(runs)
    return out


@dataclass
class Launch:
    """One gather launch as the dispatcher decides it: the fields of its name, and what the kernel is handed."""

    table: str
    kernel: str
    epilogue: str
    width: str
    k: int = 0
    padded: bool = False
    weighted: bool = True
    stripe: int = 0        # workgroups (tiles) per XCD in turn; 0: one contiguous range each
    ordered: bool = False
    vec: int = 1
    tile: int = 0          # targets per workgroup of the tiled kernels
    form: object = None    # the by-value form of the program (uniform_form / runs_form)
    head: int = 0          # fields_csr: entries the head kernel keeps in registers

    def name(self) -> str:
        return route_name(self.table, self.kernel, self.epilogue, self.width, self.k, self.padded, self.weighted, self.stripe != 0, self.ordered)


def vector_ok(T, pointers, n_lev: int, sp: int, op: int) -> bool:
    """regrid_cols_ell / regrid_cols_csr: every base on 16 bytes, both pitches whole vectors that hold the last (partial) one."""
    v = 16 // np.dtype(T).itemsize
    covered = -(-n_lev // v) * v
    return covered <= sp and covered <= op and all(p % 16 == 0 for p in pointers) and sp % v == 0 and op % v == 0


def decide_cols_ell(T, pointers, n_tgt, k, n_lev, sp, op, padded, weighted, P, host, vec_ptr, have_mask, ordered, tile_override, c: Constants = K):
    """dispatch_cols_ell and launch_cols_ell; None: the program does not fit beside the tile (ATX_SPLIT_PROGRAM)."""
    size = np.dtype(T).itemsize
    v16 = 16 // size
    vec = v16 if vector_ok(T, pointers, n_lev, sp, op) else 1
    width = "scalar" if vec == 1 else "vec"
    C = -(-n_lev // vec)
    kc = ladder_k(k, padded) if weighted else 1
    n_stage = 0 if P is None else P.shape[0]
    if kc > 0 and tile_override <= 0:
        stripe = c.long_row_stripe if (kc >= 5 and not ordered) else 0
        launch = Launch("cols_ell", "direct", "none", width, kc, padded, weighted, stripe, ordered, vec)
        if P is None:
            return launch
        form = uniform_form(T, P, have_mask, n_lev, vec, c) if host else None
        if form is not None:
            launch.epilogue, launch.form = "uniform", form
            return launch
        form = runs_form(T, P, have_mask, n_lev, c) if host else None
        if form is not None:
            launch.epilogue, launch.form = "runs", form
            return launch
        madd = (native.OP_COPY, native.OP_AFFINE, native.OP_MUL)
        if vec == v16 and host and vec_ptr is not None and vec_ptr % 16 == 0 and 1 <= n_stage <= c.max_table and all(int(e["op"]) in madd for e in P.reshape(-1)):
            launch.epilogue = "table"
            return launch
    tile = min(tile_override if tile_override > 0 else pick_tile(n_tgt, C, P is not None, c), n_tgt)
    row_bytes = k * (4 + (size if weighted else 0))
    if tile * row_bytes > c.lds_rows:
        tile = (c.lds_rows // row_bytes) // 4 * 4 if c.lds_rows // row_bytes > 4 else 1
    lds = ((tile * row_bytes + 15) & ~15) + (tables_bytes(n_stage, C, vec, size) if P is not None else 0)
    if P is not None and lds > c.lds_max:
        return None
    assert lds <= c.lds_max
    return Launch("cols_ell", "tiled", "lds" if P is not None else "none", width, kc if kc <= 4 else 0, padded, weighted, 0, ordered, vec, tile)


def decide_cols_csr(T, pointers, n_tgt, nnz, n_lev, sp, op, P, ordered, tile_override, c: Constants = K):
    """regrid_cols_csr and launch_cols_csr; None: ATX_SPLIT_PROGRAM."""
    size = np.dtype(T).itemsize
    vec = 16 // size if vector_ok(T, pointers, n_lev, sp, op) else 1
    C = -(-n_lev // vec)
    tile = min(tile_override if tile_override > 0 else pick_tile(n_tgt, C, P is not None, c), n_tgt)
    mean = nnz / n_tgt
    cap = min(int(mean * tile * 2.0) + 64, c.csr_cap)
    lds = ((cap * (size + 4) + (tile + 1) * 4 + 15) & ~15) + (tables_bytes(P.shape[0], C, vec, size) if P is not None else 0)
    if P is not None and lds > c.lds_max:
        return None
    assert lds <= c.lds_max
    stripe = c.csr_stripe if (not ordered and mean >= c.csr_stripe_min_mean) else 0
    return Launch("cols_csr", "tiled", "lds" if P is not None else "none", "scalar" if vec == 1 else "vec", 0, False, True, stripe, ordered, vec, tile)


def decide_fields_ell(k, padded, weighted, P) -> Launch:
    """dispatch_fields_ell."""
    return Launch("fields_ell", "lanes", "global" if P is not None else "none", "lane", ladder_k(k, padded, limit=4) if weighted else 1, padded, weighted)


def decide_fields_csr(n_tgt, nnz, P, c: Constants = K) -> Launch:
    """regrid_fields_csr: the head kernels up to a mean of 8 entries, 4 of them in registers up to a mean of 4."""
    mean = nnz / n_tgt
    head = 0 if mean > c.head8_mean else (4 if mean <= c.head4_mean else 8)
    return Launch("fields_csr", f"head{head}" if head else "long", "global" if P is not None else "none", "lane", head=head)


def ell_lds_fits(n_tgt, k, n_lev, dt, n_stage, c: Constants) -> bool:
    """A weighted fixed-k gather with a program of ``n_stage`` general stages on a tight aligned stack stays fused."""
    P = np.zeros((n_stage, 1), dtype=native.LEVEL_OP_DTYPE)  # (only the count of stages matters beyond kMaxUniform)
    assert n_stage > c.max_uniform
    return decide_cols_ell(dt, (), n_tgt, k, n_lev, 1 << 20, 1 << 20, False, True, P, False, None, False, False, 0, c) is not None


def csr_lds_fits(n_tgt, nnz, n_lev, dt, n_stage, c: Constants) -> bool:
    P = np.zeros((n_stage, 1), dtype=native.LEVEL_OP_DTYPE)
    return decide_cols_csr(dt, (), n_tgt, nnz, n_lev, 1 << 20, 1 << 20, P, False, 0, c) is not None


def csr_lengths(n_tgt: int, mean: int, seed: int, first=(0, 0), last=(0,)) -> tuple:
    """Row lengths around ``mean`` with empty rows first and last."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 2 * mean + 1, n_tgt)
    lengths[: len(first)] = first
    lengths[n_tgt - len(last):] = last
    return tuple(int(n) for n in lengths)


def pointwise_route_of_the_rest(n_stage: int, C: int, vec: int, size: int) -> str:
    """The per-point form that finishes a split program: in place on a tight vector-wide stack, more than kMaxUniform stages level by
    level (atx_pointwise.hip: route_levels while the per-level tables fit the 64 KB, else route_flat)."""
    if tables_bytes(n_stage, C, vec, size) + C <= 65536:
        return "levels"
    assert n_stage * C * (16 if size == 4 else 24) + C <= 65536, "the per-point pass would be cut in two: declare its second half's route"
    return "flat"


def split_cases(c: Constants) -> list:
    """kMaxStages stages over just enough levels that the tables no longer fit beside the tile: the plain gather (which for a ladder k
    is the DIRECT kernel, for k = 9 the tiled one), then the program in place through atx_pointwise_stack — and the same shape one level
    below, which stays fused.  Natural and ordered, with a mask, one stack and two."""
    out = []
    n_tgt, n_stage = 67, c.max_stages
    for dt in (np.float32, np.float64):
        t, v, size = tname(dt), vec_of(dt), np.dtype(dt).itemsize

        def program(n_lev):
            ops = (AFF, MUL, INV, DIV, CLIP, IMP)
            return tuple(tuple(m(e) if (l + s) % 5 == 0 else e for l, e in enumerate(per_level(n_lev, ops, shift=s))) for s in range(n_stage))

        lengths = csr_lengths(n_tgt, 3, seed=7)
        for table, k, fits in (("ell", 4, lambda L_: ell_lds_fits(n_tgt, 4, L_, dt, n_stage, c)), ("ell", 9, lambda L_: ell_lds_fits(n_tgt, 9, L_, dt, n_stage, c)),
                               ("csr", 0, lambda L_: csr_lds_fits(n_tgt, sum(lengths), L_, dt, n_stage, c))):
            n_lev = v
            while fits(n_lev):
                n_lev += v
            n_lev -= v - 1  # the first level of the first vector that no longer fits
            assert not fits(n_lev) and fits(n_lev - 1) and n_lev > v
            kw = dict(table=table, n_tgt=n_tgt, k=max(k, 1), lengths=lengths if table == "csr" else None, mask=1)
            pw = pointwise_route_of_the_rest(n_stage, -(-n_lev // v), v, size)
            for ordered in (False, True):
                if table == "csr":
                    gone, fused = route_name("cols_csr", "tiled", "split", "vec", ordered=ordered), route_name("cols_csr", "tiled", "lds", "vec", ordered=ordered)
                else:
                    gone, fused = (direct if k == 4 else tiled)("split", k, ordered=ordered), tiled("lds", k, ordered=ordered)
                for n_stack in ((1, 2) if k == 4 else (1,)):
                    tag = f"{table}-{t}" + (f"-k{k}" if k else "") + ("-ordered" if ordered else "") + (f"-batch{n_stack}" if n_stack > 1 else "")
                    out.append(Case(f"split-{tag}-L{n_lev}", gone, dt, n_lev=n_lev, stages=program(n_lev), ordered=ordered, n_stack=n_stack, pw_route=pw, **kw))
                    out.append(Case(f"split-stays-fused-{tag}-L{n_lev - 1}", fused, dt, n_lev=n_lev - 1, stages=program(n_lev - 1), ordered=ordered, n_stack=n_stack, **kw))
    return out


def csr_cases(c: Constants) -> list:
    """cols_csr: with and without a program; the mean row length just below and on kCsrStripeMinMean (range / stripe); tile counts below,
    on and past one group of kXcds x kCsrStripe; ordered; a tile whose entries exceed the LDS room (the read-from-L2 path); empty rows
    first and last."""
    out = []
    group = c.xcds * c.csr_stripe
    at = int(c.csr_stripe_min_mean)
    assert at == c.csr_stripe_min_mean and at >= 2
    for dt in (np.float32, np.float64):
        t, v = tname(dt), vec_of(dt)
        n_lev = 5
        prog = general_programs(n_lev, c)[f"{c.max_uniform + 1}-stages"]
        name = functools.partial(route_name, "cols_csr", "tiled")
        for i, n_tiles in enumerate((group - 1, group, group + 1)):
            n_tgt = n_tiles * 8 - (3 if i == 2 else 0)  # tiles of 8 targets (set_tuning), the last one partial past the group
            on = (0,) + (3 * at,) + (at,) * (n_tgt - 3) + (0,)  # mean exactly kCsrStripeMinMean, empty rows first and last
            below = (0,) + (3 * at - 1,) + (at,) * (n_tgt - 3) + (0,)
            assert sum(on) == at * n_tgt and sum(below) == at * n_tgt - 1
            out.append(Case(f"csr-stripe-{n_tiles}-tiles-{t}", name("none", "vec", stripe=True), dt, table="csr", n_lev=n_lev, n_tgt=n_tgt, lengths=on, tile=8))
            out.append(with_program(f"csr-stripe-{n_tiles}-tiles-program-{t}", name("lds", "vec", stripe=True), dt, prog, table="csr", n_lev=n_lev, n_tgt=n_tgt, lengths=on, tile=8))
            out.append(with_program(f"csr-range-{n_tiles}-tiles-program-{t}", name("lds", "vec"), dt, prog, table="csr", n_lev=n_lev, n_tgt=n_tgt, lengths=below, tile=8))
        on = (0,) + (3 * at,) + (at,) * (N_TGT - 3) + (0,)
        out.append(with_program(f"csr-long-rows-ordered-takes-ranges-{t}", name("lds", "vec", ordered=True), dt, prog, table="csr", n_lev=n_lev, lengths=on, ordered=True))
        out.append(Case(f"csr-long-rows-ordered-plain-{t}", name("none", "vec", ordered=True), dt, table="csr", n_lev=n_lev, lengths=on, ordered=True))
        short = csr_lengths(N_TGT, 3, seed=8)
        for n_lev_ in ((1, 3, 4, 9) if dt == np.float32 else (2, 3, 9)):
            pitch = dict(src_pitch=v, out_pitch=v) if n_lev_ == 1 else {}
            out.append(with_program(f"csr-short-rows-program-{t}-L{n_lev_}", name("lds", "vec"), dt, general_programs(n_lev_, c)[f"{c.max_stages}-stages"], table="csr", n_lev=n_lev_, lengths=short, **pitch))
        out.append(Case(f"csr-short-rows-plain-{t}", name("none", "vec"), dt, table="csr", n_lev=n_lev, lengths=short))
        out.append(with_program(f"csr-short-rows-ordered-{t}", name("lds", "vec", ordered=True), dt, prog, table="csr", n_lev=n_lev, lengths=short, ordered=True))
        out.append(with_program(f"csr-exp-log-{t}", name("lds", "vec"), dt, general_programs(9, c)["exp-log"], table="csr", n_lev=9, lengths=short))
        out.append(with_program(f"csr-one-target-{t}", name("lds", "vec"), dt, prog, table="csr", n_lev=n_lev, n_tgt=1, lengths=(3,)))
        # a few very long rows among empty ones: the tile that holds one has more entries than the LDS room for ~2x the mean
        long_rows = tuple(600 if r in (9, 70, 71) else 0 for r in range(N_TGT))
        assert int(sum(long_rows) / N_TGT * 8 * 2.0) + 64 < 600
        out.append(Case(f"csr-tile-beyond-the-lds-room-{t}", name("none", "vec", stripe=True), dt, table="csr", n_lev=n_lev, lengths=long_rows, tile=8))
        out.append(with_program(f"csr-tile-beyond-the-lds-room-program-{t}", name("lds", "vec", stripe=True), dt, prog, table="csr", n_lev=n_lev, lengths=long_rows, tile=8))
    return out


def fields_ell_cases(c: Constants) -> list:
    """fields_ell: compile-time K 1 to 4, padded 3 and 4, runtime 5 and 9 plain and padded, with and without a program, over n_lev = 1,
    kFieldsChunk, kFieldsChunk + 1 and 33 (two pick_lev_chunk chunks)."""
    out = []
    levels = (1, c.fields_chunk, c.fields_chunk + 1, 33)
    variants = [(1, False, False), (1, False, True), (2, False, True), (3, False, True), (4, False, True), (3, True, True), (4, True, True), (5, False, True),
                (5, True, True), (9, False, True), (9, True, True), (2, True, True)]
    for dt in (np.float32, np.float64):
        t = tname(dt)
        for i, (k, padded, weighted) in enumerate(variants):
            tag = f"k{k}" + ("-padded" if padded else "") + ("" if weighted else "-pure")
            kk = ladder_k(k, padded, limit=4) if weighted else 1
            for j, n_lev in enumerate(levels if k in (4, 9) and not padded else (levels[(i + 1) % 4], levels[(i + 2) % 4])):
                n_tgt = (N_TGT, c.block, c.block + 1, 1)[(i + j) % 4]
                name = functools.partial(route_name, "fields_ell", "lanes", width="lane", k=kk, padded=padded, weighted=weighted)
                prog = general_programs(n_lev, c)[f"{c.max_uniform + 1 + (i + j) % 4}-stages"]
                out.append(with_program(f"fields-ell-{t}-{tag}-L{n_lev}-N{n_tgt}-program", name(epilogue="global"), dt, prog, layout=FIELDS, n_lev=n_lev, n_tgt=n_tgt, k=k, padded=padded,
                                        weighted=weighted, n_stack=1 + (i + j) % 2))
                if j == 0:
                    out.append(Case(f"fields-ell-{t}-{tag}-L{n_lev}-N{n_tgt}", name(epilogue="none"), dt, layout=FIELDS, n_lev=n_lev, n_tgt=n_tgt, k=k, padded=padded, weighted=weighted))
        out.append(with_program(f"fields-ell-{t}-k4-exp-log", route_name("fields_ell", "lanes", "global", "lane", 4), dt, general_programs(9, c)["exp-log"], layout=FIELDS, n_lev=9, k=4))
        out.append(with_program(f"fields-ell-{t}-k9-odd-pitch", route_name("fields_ell", "lanes", "global", "lane", 0), dt, general_programs(5, c)[f"{c.max_stages}-stages"], layout=FIELDS, n_lev=5, k=9,
                                src_pitch=N_SRC + 1, out_pitch=N_TGT + 2, offset=1))
    return out


def head_lengths(n_tgt: int, R: int, mean_at_most: float, mean_above: float) -> tuple:
    """Rows of exactly R, R + 1 and 0 entries and one of several times R, the rest short enough to keep the mean in (mean_above, mean_at_most]."""
    lengths = [R, R + 1, 0, 3 * R + 1] + [0] * (n_tgt - 4)
    target = int(mean_at_most * n_tgt)  # the largest nnz with mean <= mean_at_most
    i = 4
    while sum(lengths) < target:
        lengths[4 + (i - 4) % (n_tgt - 4)] += 1
        i += 1
    assert mean_above < sum(lengths) / n_tgt <= mean_at_most, (sum(lengths) / n_tgt, mean_above, mean_at_most)
    return tuple(lengths)


def fields_csr_cases(c: Constants) -> list:
    """fields_csr head4, head8 and long, chosen by the mean on its boundary: each with rows of exactly R, R + 1 and 0 entries and one
    several times R (the head kernels' tail loop inside a launch whose mean is small), with and without a program."""
    out = []
    levels = (1, c.fields_chunk, c.fields_chunk + 1, 33)
    for dt in (np.float32, np.float64):
        t = tname(dt)
        for kern, R, hi, lo in (("head4", 4, c.head4_mean, 0.0), ("head8", 8, c.head8_mean, c.head4_mean), ("long", 8, 2 * c.head8_mean, c.head8_mean)):
            for j, n_lev in enumerate(levels):
                n_tgt = (N_TGT, c.block, c.block + 1, 37)[j]
                lengths = head_lengths(n_tgt, R, hi, lo)
                if kern == "head8" and j % 2:  # just past head4's mean: one entry more than its largest nnz
                    lengths = head_lengths(n_tgt, R, c.head4_mean, 0.0)
                    lengths = lengths[:5] + (lengths[5] + 1,) + lengths[6:]
                    assert sum(lengths) / n_tgt > c.head4_mean
                if kern == "long" and j % 2:  # just past head8's
                    lengths = head_lengths(n_tgt, R, c.head8_mean, c.head4_mean)
                    lengths = lengths[:5] + (lengths[5] + 1,) + lengths[6:]
                    assert sum(lengths) / n_tgt > c.head8_mean
                name = functools.partial(route_name, "fields_csr", kern, width="lane")
                prog = general_programs(n_lev, c)[f"{c.max_uniform + 1 + j}-stages"]
                out.append(with_program(f"fields-csr-{kern}-{t}-L{n_lev}-N{n_tgt}-program", name(epilogue="global"), dt, prog, table="csr", layout=FIELDS, n_lev=n_lev, n_tgt=n_tgt, lengths=lengths))
                if j % 2 == 0:
                    out.append(Case(f"fields-csr-{kern}-{t}-L{n_lev}-N{n_tgt}", name(epilogue="none"), dt, table="csr", layout=FIELDS, n_lev=n_lev, n_tgt=n_tgt, lengths=lengths))
            out.append(with_program(f"fields-csr-{kern}-{t}-exp-log", route_name("fields_csr", kern, "global", "lane"), dt, general_programs(9, c)["exp-log"], table="csr", layout=FIELDS, n_lev=9,
                                    lengths=head_lengths(N_TGT, R, hi, lo)))
    return out


def all_cases(c: Constants = K) -> list:
    cases = (direct_epilogue_cases(c) + shape_cases(c) + loose_pitch_cases(c) + tiled_cases(c) + scalar_cases(c) + split_cases(c) + csr_cases(c) + fields_ell_cases(c) + fields_csr_cases(c))
    names = [case.name for case in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    groups = {}
    for case in cases:
        if case.group:
            assert groups.setdefault(case.group, case.problem_key()) == case.problem_key(), f"{case.name}: another problem than its group's"
    return cases


def declared_route_classes(cases) -> set:
    return {route_class(case.route) for case in cases}


# ---- the problem of a case: sources, tables, the mask, and what scipy and numpy make of them ---------------------------------------
def make_sources(rng, dt, n_lev, n_src, every: int) -> np.ndarray:
    """[n_lev, n_src]: values around 280, one in four around 0 (finite exponentials in float32), every ``every``-th element a special one."""
    x = (280.0 + 30.0 * rng.standard_normal((n_lev, n_src))).astype(dt)
    small = rng.random(x.shape) < 0.25
    x[small] = (3.0 * rng.standard_normal(int(small.sum()))).astype(dt)
    flat = x.reshape(-1)
    sp = special_values(dt)
    at = np.arange(1 if flat.size > 1 else 0, flat.size, every)
    shift = int(rng.integers(0, sp.size))
    flat.view(bits_type(dt))[at] = sp.view(bits_type(dt))[(np.arange(at.size) + shift) % sp.size]
    return x


def make_weights(rng, dt, shape) -> np.ndarray:
    """Rows that sum to about 1, one entry in ten negative and one in ten exactly 0."""
    w = rng.random(shape) + 0.05
    w = w / w.sum(axis=-1, keepdims=True) if len(shape) == 2 else w / 3.0
    draw = rng.random(shape)
    w = np.where(draw < 0.1, -w, np.where(draw < 0.2, 0.0, w))
    return w.astype(dt)


def padded_rows(rng, idx, w):
    """As ``padded_table`` of tests/test_gpu_regrid_routes.py — rows of 0..k present entries anywhere in the row, the first three the all-absent
    row, the full one and a single entry in the last slot — and every absent entry keeps a weight that must not be used."""
    n_tgt, k = idx.shape
    lengths = rng.integers(0, k + 1, size=n_tgt)
    first = (0, k, 1) if n_tgt >= 3 else (1,)
    lengths[: len(first)] = first[:n_tgt]
    present = np.stack([rng.permutation(k) < n for n in lengths])
    present[min(2, n_tgt - 1)] = np.arange(k) == k - 1
    return np.where(present, idx, -1).astype(np.int32), np.where(present | (rng.random(idx.shape) < 0.5), w, 0).astype(w.dtype)


def make_mask(rng, n_tgt: int) -> np.ndarray:
    set_ = rng.random(n_tgt) < 0.4
    if n_tgt > 1:
        set_[:2] = [True, False]
        set_[-1] = False  # (the bytes before the first and after the last point are set)
    return np.where(set_, np.array([1, 2, 128, 255], dtype=np.uint8)[np.arange(n_tgt) % 4], 0).astype(np.uint8)


@dataclass
class Problem:
    xs: list                  # n_stack x [n_lev, n_src]
    idx: Optional[np.ndarray]  # ell: [n_tgt, k] int32 (-1: absent)
    w: Optional[np.ndarray]
    indptr: np.ndarray        # the CSR form of either table, what scipy is given
    indices: np.ndarray
    data: Optional[np.ndarray]
    order: np.ndarray         # the visiting order of an ordered launch: table row t is output row order[t]
    mask: Optional[np.ndarray]
    gathered: list            # n_stack x [n_lev, n_tgt]: scipy's csr_matvec (or the indexing of the pure gather)
    want: list                # ... then numpy's statements
    args: list                # ... and the arguments of the exp / log levels


@functools.lru_cache(maxsize=None)
def _problem(key: tuple) -> Problem:
    seed_name, dt, table, n_lev, n_tgt, n_src, k, padded, weighted, n_stack, stages, has_mask, lengths = key
    rng = np.random.default_rng(zlib.crc32(seed_name.encode()))
    if table == "ell":
        idx = rng.integers(0, n_src, size=(n_tgt, k)).astype(np.int32)
        w = make_weights(rng, dt, (n_tgt, k)) if weighted else None
        if padded:
            idx, w = padded_rows(rng, idx, w)
        present = idx >= 0
        indptr = np.concatenate([[0], np.cumsum(present.sum(axis=1))]).astype(np.int32)
        indices, data = idx[present], (w[present] if weighted else None)
        per_row = k
    else:
        idx = w = None
        indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        nnz = int(indptr[-1])
        indices = rng.integers(0, n_src, size=nnz).astype(np.int32)
        data = make_weights(rng, dt, (nnz,))
        per_row = max(1, -(-nnz // n_tgt))
    xs = [make_sources(rng, dt, n_lev, n_src, 3 * per_row + 1) for _ in range(n_stack)]
    order = rng.permutation(n_tgt).astype(np.int32)
    mask = make_mask(rng, n_tgt) if has_mask else None
    gathered, want, args = [], [], []
    with np.errstate(all="ignore"):
        for x in xs:
            if weighted:
                g = np.stack([oracle.csr_apply(data, indices, indptr, (n_tgt, n_src), np.ascontiguousarray(f)) for f in x])
            else:
                g = oracle.gather_nn(x, idx[:, 0])
            assert g.dtype == dt
            gathered.append(g)
            if stages is None:
                want.append(g)
                args.append({})
            else:
                y, a = reference(g, stages, mask)
                want.append(y)
                args.append(a)
    for a in xs + gathered + want + [idx, w, indptr, indices, data, order, mask]:
        if a is not None:
            a.setflags(write=False)
    return Problem(xs, idx, w, indptr, indices, data, order, mask, gathered, want, args)


def problem(case: Case) -> Problem:
    return _problem(case.problem_key())


# ---- storage --------------------------------------------------------------------------------------------------------------------
class Buffer:
    """``n_rows`` rows ``pitch`` apart, ``offset`` elements into a 16-byte aligned allocation, canary rows before and after.  Everything that
    is no level holds the poison pattern; the levels of an output hold a finite value no result takes, so an element never written shows."""

    def __init__(self, case: Case, n_pts: int, pitch: int, offset: int, device, values: Optional[np.ndarray], fill: float = 12345.0):
        dt, v = case.np_dtype, case.vec
        self.dt, self.layout, self.pitch = dt, case.layout, pitch
        self.n_rows, self.row_len = (n_pts, case.n_lev) if case.layout == COLUMNS else (case.n_lev, n_pts)
        guard = (-(-max(pitch, self.row_len) // v) + 1) * v
        self.base = guard + offset
        host = poison_bits(dt, self.base + self.n_rows * pitch + guard, values is None).view(dt)
        rows = host[self.base: self.base + self.n_rows * pitch].reshape(self.n_rows, pitch)
        if values is None:
            rows[:, : self.row_len] = fill
        else:
            rows[:, : self.row_len] = values.T if case.layout == COLUMNS else values
        self.before = host.view(bits_type(dt)).copy()
        self.backing = torch.from_numpy(host).to(device)
        assert self.backing.data_ptr() % 16 == 0
        self.view = self.backing[self.base:]
        assert (self.view.data_ptr() % 16 == 0) == (offset % v == 0)

    def bits(self) -> np.ndarray:
        return self.backing.cpu().numpy().view(bits_type(self.dt))

    def split(self, bits: np.ndarray):
        """(levels [n_lev, n_pts], what the call may not touch: a boolean over the whole allocation)."""
        rows = bits[self.base: self.base + self.n_rows * self.pitch].reshape(self.n_rows, self.pitch)
        levels = rows[:, : self.row_len].T if self.layout == COLUMNS else rows[:, : self.row_len]
        keep = np.ones(bits.size, dtype=bool)
        own_ = keep[self.base: self.base + self.n_rows * self.pitch].reshape(self.n_rows, self.pitch)
        # column stacks: the rest of the 16-byte vector that holds the last level is unspecified (include/atx.h), where the pitch has it
        v = 16 // np.dtype(self.dt).itemsize
        own_[:, : min(-(-self.row_len // v) * v, self.pitch) if self.layout == COLUMNS else self.row_len] = False
        return levels.copy(), keep


class Table:
    """A read-only device array and what it held."""

    def __init__(self, host: np.ndarray, device, lead: int = 0, surround=None):
        alloc = host.reshape(-1) if surround is None else np.concatenate([np.full(lead, surround, host.dtype), host.reshape(-1), np.full(16, surround, host.dtype)])
        self.before = alloc.copy()
        self.backing = torch.from_numpy(self.before.copy()).to(device)
        self.view = self.backing[lead: lead + host.size] if surround is not None else self.backing

    def unchanged(self) -> bool:
        return np.array_equal(self.backing.cpu().numpy().view(np.uint8), self.before.view(np.uint8))


def build_program(kern: Kernels, case: Case, device):
    if case.stages is None:
        return None
    prog = kern.level_program([list(st) for st in case.stages], device)
    for name in case.strip:
        if name == "host_prog":
            prog.host_prog = None
        else:
            assert name == "vec_prog"
            prog.vec_prog = {}
    return prog


# ---- the check ------------------------------------------------------------------------------------------------------------------
GROUPS: dict = {}  # group -> (case name, the bits of every output): the first case of a group to run is what the others must match


def check_case(kern: Kernels, device, case: Case, groups: Optional[dict] = None) -> str:
    """Run the case; returns the route taken."""
    dt = case.np_dtype
    groups = GROUPS if groups is None else groups
    uses_mask = case.stages is not None and any(e[1] for st in case.stages for e in st)
    assert case.mask is not None or not uses_mask, case.name
    assert case.ordered is False or case.layout == COLUMNS
    p = problem(case)
    n_tgt, n_src, n_lev = case.n_tgt, case.n_src, case.n_lev
    srcs = [Buffer(case, n_src, case.sp(), 0, device, x) for x in p.xs]
    outs = [Buffer(case, n_tgt, case.op(), case.offset, device, None) for _ in p.xs]
    mask = None if p.mask is None else Table(p.mask, device, lead=case.mask, surround=255)
    rows = Table(p.order, device) if case.ordered else None
    visit = p.order if case.ordered else np.arange(n_tgt)  # table row t holds the entries of output row visit[t]
    prog = build_program(kern, case, device)
    kw = dict(n_src=n_src, n_tgt=n_tgt, n_lev=n_lev, src_pitch=case.sp(), out_pitch=case.op(), layout=case.layout, prog=prog,
              n_stage=0 if case.stages is None else len(case.stages), tgt_mask=None if mask is None else mask.view, tgt_rows=None if rows is None else rows.view)
    if case.table == "ell":
        tables = [Table(np.ascontiguousarray(p.idx[visit]), device)] + ([Table(np.ascontiguousarray(p.w[visit]), device)] if case.weighted else [])
    else:
        lengths = np.diff(p.indptr)[visit]
        indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        take = np.concatenate([np.arange(p.indptr[r], p.indptr[r + 1]) for r in visit] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        tables = [Table(indptr, device), Table(np.ascontiguousarray(p.indices[take]), device), Table(np.ascontiguousarray(p.data[take]), device)]
    kern.set_tuning(case.tile)
    try:
        if case.table == "ell":
            args = (tables[0].view, tables[1].view if case.weighted else None)
            if case.n_stack == 1:
                kern.regrid_ell(srcs[0].view, outs[0].view, *args, k=case.k, padded=case.padded, **kw)
            else:
                kern.regrid_ell_batch([s.view for s in srcs], [o.view for o in outs], *args, k=case.k, padded=case.padded, **kw)
        else:
            assert case.n_stack == 1
            kern.regrid_csr(srcs[0].view, outs[0].view, tables[0].view, tables[1].view, tables[2].view, nnz=int(p.indptr[-1]), **kw)
    finally:
        kern.set_tuning(0)
    route = kern.last_gather_route()
    assert route == case.route, f"{case.name}: route {route}, the case is written for {case.route}"
    if case.pw_route is not None:
        assert kern.last_route() == case.pw_route, f"{case.name}: the program was finished by the per-point form {kern.last_route()}, the case is written for {case.pw_route}"
    taken = []
    for i, (src, out) in enumerate(zip(srcs, outs)):
        what = f"{case.name} [{route}]" + (f" stack {i}" if case.n_stack > 1 else "")
        after = out.bits()
        levels, keep = out.split(after)
        taken.append(levels)
        stages = case.stages if case.stages is not None else ((CP,) * n_lev,)
        # a weighted sum is arithmetic whatever follows: where scipy has a NaN, a NaN (the payload of a NaN that an addition made is the machine's)
        compare_levels(dt, stages, levels, p.gathered[i], p.want[i], p.args[i], what, copies_are_bit_copies=not case.weighted)
        moved = keep & (after != out.before)
        if moved.any():
            at = int(np.flatnonzero(moved)[0]) - out.base
            row, col = divmod(at, out.pitch)
            inside = 0 <= at < out.n_rows * out.pitch
            where = f"row {row} element {col} (pitch {out.pitch}, row length {out.row_len})" if inside else f"element {at} from the base"
            raise AssertionError(f"{what}: {'padding' if inside else 'canary'} written: {where} holds {int(after[at + out.base]):#x}")
        assert np.array_equal(src.bits(), src.before), f"{what}: the source stack was changed"
    for name, t in zip(("idx / indptr", "w / indices", "data"), tables):
        assert t.unchanged(), f"{case.name}: the table {name} was written"
    assert rows is None or rows.unchanged(), f"{case.name}: tgt_rows was written"
    assert mask is None or mask.unchanged(), f"{case.name}: the mask was written"
    if case.group:
        first_name, first = groups.setdefault(case.group, (case.name, taken))
        for i, (a, b) in enumerate(zip(taken, first)):
            same = a == b
            assert same.all(), f"{case.name} [{route}]: differs from {first_name}, which ran the same problem — {first_difference(a.view(dt), b.view(dt), ~same)}"
    return route


def check_nothing_launched(kern: Kernels, device) -> None:
    """A gather without targets launches nothing: ``none``, after a call that did launch."""
    case = Case("one-target", direct("none", 4), np.float32, n_lev=4, n_tgt=1)
    check_case(kern, device, case)
    p = problem(case)
    src, out = Buffer(case, case.n_src, 4, 0, device, p.xs[0]), Buffer(case, 1, 4, 0, device, None)
    idx, w = Table(p.idx, device), Table(p.w, device)
    kern.regrid_ell(src.view, out.view, idx.view, w.view, n_src=case.n_src, n_tgt=0, k=4, n_lev=4, src_pitch=4, out_pitch=4, layout=COLUMNS)
    assert kern.last_gather_route() == "none", f"no targets: route {kern.last_gather_route()}"
    assert np.array_equal(out.bits(), out.before), "no targets: the output was written"
