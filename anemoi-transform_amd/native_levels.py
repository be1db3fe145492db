"""ctypes binding of libatx_levels — the model levels of a stack of variables interpolated to pressure levels, one column at a time
(``include/atx_levels.h``), a library of its own next to libatx.

There is no CPU fallback: if ``lib/libatx_levels.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call raises.
Return codes map to the exception types of ``native``: ``ValueError``, ``AssertionError`` (shapes), ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes
from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Any

import torch

from ._binding import Library
from .native import EINVAL, ENOTIMPL, ESHAPE, OK, AtxError, _ptr, _stream, dtype_code  # noqa: F401 - OK is one of this module's names

LINEAR, LOG = 0, 1  # atx_levels_coordinate
COORDINATES = {"linear": LINEAR, "log": LOG}
NEAREST, MISSING = 0, 1  # atx_levels_outside
OUTSIDE = {"nearest": NEAREST, "missing": MISSING}
MAX_LEVELS = 256  # ATX_LEVELS_MAX_LEVELS

# every symbol include/atx_levels.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_levels_version": (c_int, []),
    "atx_levels_last_error": (c_char_p, []),
    "atx_levels_interpolate": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int,
         c_int, c_int, c_int, c_void_p],
    ),
}

LIBRARY = Library("libatx_levels.so", "ATX_LEVELS_LIBRARY", SIGNATURES, "atx_levels_last_error",
                  errors={EINVAL: ValueError, ESHAPE: AssertionError, ENOTIMPL: NotImplementedError},
                  unmapped=lambda fn, message, code: AtxError(f"{fn}: {message} (code {code})"))
lib_path = LIBRARY.path  # ``lib/libatx_levels.so`` next to this file; ``ATX_LEVELS_LIBRARY`` overrides it
load = LIBRARY.load  # libatx_levels.so, opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def _call(fn: str, *args: Any) -> None:
    LIBRARY.check(fn, getattr(load(), fn)(*args))


def _code(value, table: dict[str, int], what: str) -> int:
    """A name of ``table`` (or the enum value itself) as the enum value."""
    if isinstance(value, str):
        if value not in table:
            raise ValueError(f"unknown {what} {value!r}: one of {', '.join(table)}")
        return table[value]
    return int(value)


def coordinate_code(coordinate) -> int:
    """``"linear"`` / ``"log"`` (or the enum value itself) as ``atx_levels_coordinate``."""
    return _code(coordinate, COORDINATES, "coordinate")


def outside_code(outside) -> int:
    """``"nearest"`` / ``"missing"`` (or the enum value itself) as ``atx_levels_outside``."""
    return _code(outside, OUTSIDE, "outside policy")


def interpolate(src, out, sp, A, B, targets, *, n_pts, n_var, n_lev, n_tgt, src_pitch, out_pitch, layout, level_index=None,
                coordinate="linear", outside="nearest") -> None:
    """``n_var`` variables of ``n_lev`` model levels each to the ``n_tgt`` pressures of ``targets`` (Pa) for every point
    (``atx_levels_interpolate``, include/atx_levels.h holds the statement).  ``src`` / ``out`` / ``sp`` share a type; ``A`` / ``B`` /
    ``targets`` are float64 device tensors; ``level_index`` is a HOST sequence of the rows' 0-based model levels (``None``: ``0 .. n_lev - 1``)."""
    assert src.dtype == out.dtype == sp.dtype, (src.dtype, out.dtype, sp.dtype)
    assert A.dtype == B.dtype == targets.dtype == torch.float64, (A.dtype, B.dtype, targets.dtype)
    assert A.numel() == B.numel() and targets.numel() == n_tgt and sp.numel() == n_pts and sp.is_contiguous()
    index = None
    if level_index is not None:
        levels = [int(m) for m in level_index]
        assert len(levels) == n_lev, (len(levels), n_lev)
        index = (ctypes.c_int32 * max(1, n_lev))(*levels)
    _call("atx_levels_interpolate", _ptr(src), _ptr(out), _ptr(sp), _ptr(A), _ptr(B), index, _ptr(targets), n_pts, n_var, n_lev, n_tgt, A.numel(),
          src_pitch, out_pitch, dtype_code(src.dtype), layout, coordinate_code(coordinate), outside_code(outside), _stream())
