"""What a level of a per-level program must hold, for the checks that compare a kernel with numpy (tests/pointwise_route_checks.py: the
per-point launch forms; tests/gather_route_checks.py: the gather's fused epilogues): the operators the cases are built from, the special
values the inputs carry, the poison pattern of padding and canaries, numpy's statements stage by stage (``reference``) and the comparison
of every level (``compare_levels``) —

- a level whose stages are all plain COPY: a bit copy (NaN payloads, signalling NaNs and -0.0 included);
- an arithmetic level: numpy's bits in the stack's own dtype (``native_double._apply_op``: one rounding per ufunc, parameters rounded as
  ``np.float32(p)`` / ``np.float64(p)``); where numpy gives a NaN, a NaN.  float32 exactly as float64;
- an EXP / LOG level: the exact function (tests/exact_statements.py) of the argument as the stages before it leave it, within the budget
  tests/ulp_budgets.py derives for the operator.  No number of its own here.
"""

from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

import exact_statements as X
import native_double
from anemoi_transform_amd import native
from ulp_budgets import budgets

# ---- programs -----------------------------------------------------------------------------------------------------------------
CP = (native.OP_COPY, 0, 0.0, 0.0)
AFF = (native.OP_AFFINE, 0, 1.5, -3.0)
TAFF = (native.OP_AFFINE, 0, 0.03125, -6.0)  # ahead of exp / log: 280 -> 2.75
MUL = (native.OP_MUL, 0, 9.80665, 0.0)
INV = (native.OP_AFFINE_INV, 0, 2.0, 1.0)
DIV = (native.OP_DIV, 0, 9.80665, 0.0)
CLIP = (native.OP_CLIP, 0, 250.0, 300.0)
CLIP_LO = (native.OP_CLIP, 0, -20.0, math.nan)  # no upper bound
CLIP_HI = (native.OP_CLIP, 0, math.nan, 40.0)
IMP = (native.OP_IMPUTE_NAN, 0, -1.0, 0.0)
EXP = (native.OP_EXP, 0, 0.0, 0.0)
LOG = (native.OP_LOG, 0, 0.0, 0.0)
SETNAN = (native.OP_SET_NAN, 0, 0.0, 0.0)
MSK = (native.OP_COPY, 1, 0.0, 0.0)
CLIP_BOUNDS = (250.0, 300.0, -20.0, 40.0)
ARITH = (AFF, MUL, INV, DIV, CLIP, IMP, CLIP_LO, CLIP_HI)


def m(e):
    """The operator with the point mask."""
    return (e[0], 1, e[2], e[3])


def own(e, l):
    """The operator with parameters of level ``l``'s own (never a clip: its bounds stay the ones the inputs straddle)."""
    if e[0] in (native.OP_CLIP, native.OP_COPY, native.OP_EXP, native.OP_LOG, native.OP_SET_NAN):
        return e
    return (e[0], e[1], e[2] * (1.0 + 0.03125 * (l % 7 + 1)), e[3] + 0.5 * (l % 5))


def pieces(n_lev, *parts):
    """A stage from ``(first level, operator)`` runs: ``pieces(9, (0, AFF), (4, MUL))``."""
    starts = [p[0] for p in parts] + [n_lev]
    assert starts[0] == 0 and all(a < b for a, b in zip(starts, starts[1:])), starts
    return tuple(e for (a, e), b in zip(parts, starts[1:]) for _ in range(b - a))


def per_vector(n_lev, vec, ops):
    """One operator per 16-byte vector of levels, the next one in the next vector."""
    return tuple(ops[(l // vec) % len(ops)] for l in range(n_lev))


def per_level(n_lev, ops, shift=0):
    """Operators that change inside every vector, each level with parameters of its own."""
    return tuple(own(ops[(l + shift) % len(ops)], l) for l in range(n_lev))


def tname(dt) -> str:
    return "f32" if dt == np.float32 else "f64"


def vec_of(dt) -> int:
    return 4 if dt == np.float32 else 2


def torch_dtype(dt):
    return torch.float32 if dt == np.float32 else torch.float64


# ---- values, reference ----------------------------------------------------------------------------------------------------------
def bits_type(dt):
    return np.uint32 if dt == np.float32 else np.uint64


def from_bits(dt, *patterns) -> np.ndarray:
    return np.array(patterns, dtype=bits_type(dt)).view(dt)


def poison_bits(dt, n: int, output: bool) -> np.ndarray:
    """What padding and canaries hold: a quiet NaN with a payload of its own and a finite value nothing computes, in turn (an
    operator applied to padding in place changes one of the two), the other way round and with another payload in an output (a
    copy of the input's padding shows)."""
    nan, finite = (0x7FC5A5A5, 0x7FC3C3C3), np.array([1.2345e30, -5.4321e29], dtype=dt).view(bits_type(dt))
    if dt == np.float64:
        nan = (0x7FF8A5A5A5A5A5A5, 0x7FF8C3C3C3C3C3C3)
    pattern = np.array([nan[1], finite[1]] if output else [finite[0], nan[0]], dtype=bits_type(dt))
    return pattern[np.arange(n) % 2]


def special_values(dt) -> np.ndarray:
    fin = np.finfo(dt)
    nans = from_bits(dt, 0x7FC12345, 0xFF812345) if dt == np.float32 else from_bits(dt, 0x7FF8000000012345, 0xFFF0000000012345)
    around = [f(dt(b), dt(s)) for b in CLIP_BOUNDS for f, s in ((np.nextafter, -np.inf), (lambda a, _: a, 0), (np.nextafter, np.inf))]
    plain = np.array([0.0, -0.0, np.inf, -np.inf, fin.smallest_subnormal, -3 * fin.smallest_subnormal, fin.tiny, fin.max, -fin.max] + around, dtype=dt)
    return np.concatenate([nans, plain])


def entry_of(e) -> np.ndarray:
    entry = np.zeros((), dtype=native.LEVEL_OP_DTYPE)
    entry["op"], entry["use_mask"], entry["p0"], entry["p1"] = e
    return entry


def plain_copy(e) -> bool:
    return e[0] == native.OP_COPY and not e[1]


def level_kind(stages, l):
    """("copy" | "arith", None) or ("exp" | "log", the stage): an exp / log level has one such stage and only plain COPY after it."""
    col = [st[l] for st in stages]
    trans = [s for s, e in enumerate(col) if e[0] in (native.OP_EXP, native.OP_LOG)]
    if trans:
        assert len(trans) == 1 and all(plain_copy(e) for e in col[trans[0] + 1:]), "an exp / log level ends with it"
        return ("exp" if col[trans[0]][0] == native.OP_EXP else "log"), trans[0]
    return ("copy" if all(plain_copy(e) for e in col) else "arith"), None


def reference(x: np.ndarray, stages, mask: Optional[np.ndarray]):
    """numpy's statements, stage by stage; also the argument every exp / log level hands to its function."""
    want = x.copy()
    args = {}
    set_ = None if mask is None else mask != 0
    with np.errstate(all="ignore"):
        for s, stage in enumerate(stages):
            for l, e in enumerate(stage):
                if plain_copy(e):
                    continue
                if e[0] in (native.OP_EXP, native.OP_LOG):
                    args[l] = want[l].copy()
                assert not e[1] or set_ is not None, "the program uses a mask the case does not give"
                want[l] = native_double._apply_op(entry_of(e), want[l].copy(), set_ if e[1] else None)
    return want, args


# ---- the comparison -------------------------------------------------------------------------------------------------------------
def first_difference(got, want, where):
    l, p = np.argwhere(where)[0]
    return f"level {l} point {p}: kernel {got[l, p]!r} ({int(got[l, p].view(bits_type(got.dtype.type))):#x}), numpy {want[l, p]!r} ({int(want[l, p].view(bits_type(got.dtype.type))):#x})"


def compare_levels(dt, stages, got_bits: np.ndarray, x: np.ndarray, want: np.ndarray, args: dict, what: str, copies_are_bit_copies: bool = True):
    """``got_bits`` [n_lev, n_pts] against the expectation of every level: ``x`` is what a level of plain COPY stages must be a bit copy
    of, ``want`` / ``args`` come from ``reference``.  ``copies_are_bit_copies=False``: ``x`` is itself the result of arithmetic (a weighted
    sum), so such a level is held like an arithmetic one — numpy's bits, and a NaN where numpy has one, whatever its payload."""
    got = got_bits.view(dt)
    want_bits, x_bits = want.view(bits_type(dt)), x.view(bits_type(dt))
    kinds = [level_kind(stages, l) for l in range(len(stages[0]))]
    copy = np.array([k == "copy" and copies_are_bit_copies for k, _ in kinds])
    arith = np.array([k == "arith" or (k == "copy" and not copies_are_bit_copies) for k, _ in kinds])
    wrong = np.zeros(got.shape, dtype=bool)
    wrong[copy] = got_bits[copy] != x_bits[copy]
    assert not wrong.any(), f"{what}: a level of plain COPY stages is no bit copy of the input — {first_difference(got, x, wrong)}"
    nan = np.isnan(want)
    wrong[arith] = np.isnan(got[arith]) != nan[arith]
    assert not wrong.any(), f"{what}: NaN where numpy has none, or none where numpy has one — {first_difference(got, want, wrong)}"
    wrong[arith] = (got_bits[arith] != want_bits[arith]) & ~nan[arith]
    assert not wrong.any(), f"{what}: {int(wrong.sum())} values differ from numpy's bits — {first_difference(got, want, wrong)}"
    for l, (kind, _) in enumerate(kinds):
        if kind in ("exp", "log"):
            exact = X.exact_values(X.exp_exact if kind == "exp" else X.log_exact, args[l])
            err = X.ulp_errors(got[l], exact, dt)
            bound = budgets(dt)[(kind, 0)]
            i = int(np.argmax(err))
            assert err.max() <= bound, f"{what}: {kind} level {l}: {err.max():.3f} ulps > {bound} at point {i}, argument {args[l][i]!r}, kernel {got[l, i]!r}"
