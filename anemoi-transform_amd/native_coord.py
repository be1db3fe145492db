"""ctypes binding of libatx_coord — the variables of a stack of levels interpolated onto surfaces of a second stack's values, the
per-point coordinate column read from memory (``include/atx_coord.h``), a library of its own next to libatx and the other vertical
libraries.

There is no CPU fallback: if ``lib/libatx_coord.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call raises.
Return codes map to the exception types of ``native``: ``ValueError``, ``AssertionError`` (shapes), ``NotImplementedError``.
"""

from __future__ import annotations

from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Any

import torch

from ._binding import Library
from .native import EINVAL, ENOTIMPL, ESHAPE, OK, AtxError, _ptr, _stream, dtype_code  # noqa: F401 - OK is one of this module's names

NEAREST, MISSING = 0, 1  # atx_coord_outside
OUTSIDE = {"nearest": NEAREST, "missing": MISSING}
MAX_LEVELS = 256  # ATX_COORD_MAX_LEVELS
ULPS_F64 = 11  # ATX_COORD_ULPS_F64

# every symbol include/atx_coord.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_coord_version": (c_int, []),
    "atx_coord_last_error": (c_char_p, []),
    "atx_coord_interpolate": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int,
         c_int, c_int, c_void_p],
    ),
}

LIBRARY = Library("libatx_coord.so", "ATX_COORD_LIBRARY", SIGNATURES, "atx_coord_last_error",
                  errors={EINVAL: ValueError, ESHAPE: AssertionError, ENOTIMPL: NotImplementedError},
                  unmapped=lambda fn, message, code: AtxError(f"{fn}: {message} (code {code})"))
lib_path = LIBRARY.path  # ``lib/libatx_coord.so`` next to this file; ``ATX_COORD_LIBRARY`` overrides it
load = LIBRARY.load  # opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def _call(fn: str, *args: Any) -> None:
    LIBRARY.check(fn, getattr(load(), fn)(*args))


def outside_code(outside) -> int:
    """``"nearest"`` / ``"missing"`` (or the enum value itself) as ``atx_coord_outside``."""
    if isinstance(outside, str):
        if outside not in OUTSIDE:
            raise ValueError(f"unknown outside policy {outside!r}: one of {', '.join(OUTSIDE)}")
        return OUTSIDE[outside]
    return int(outside)


def interpolate(src, coord, out, targets, *, n_pts, n_var, n_lev, n_tgt, src_pitch, coord_pitch, out_pitch, layout, offset=None, floor=None,
                bad=None, outside="nearest") -> None:
    """``n_var`` variables of ``n_lev`` levels each to the ``n_tgt`` surfaces ``coord == targets[t] (+ offset)`` for every point
    (``atx_coord_interpolate``, include/atx_coord.h holds the statement).  ``src`` / ``coord`` / ``out`` / ``offset`` / ``floor`` share a
    type; ``targets`` is a float64 device tensor; ``bad`` a uint8 device tensor of ``n_pts``.  Every pointer is a device pointer."""
    assert src.dtype == coord.dtype == out.dtype, (src.dtype, coord.dtype, out.dtype)
    assert targets.dtype == torch.float64 and targets.numel() == n_tgt, (targets.dtype, targets.numel())
    for name, vector in (("offset", offset), ("floor", floor)):
        if vector is not None:
            assert vector.dtype == src.dtype and vector.numel() == n_pts and vector.is_contiguous(), (name, vector.dtype, vector.numel())
    if bad is not None:
        assert bad.dtype == torch.uint8 and bad.numel() == n_pts and bad.is_contiguous(), (bad.dtype, bad.numel())
    optional = lambda x: None if x is None else _ptr(x)  # noqa: E731
    _call("atx_coord_interpolate", _ptr(src), _ptr(coord), _ptr(out), optional(offset), optional(floor), optional(bad), _ptr(targets), n_pts, n_var,
          n_lev, n_tgt, src_pitch, coord_pitch, out_pitch, dtype_code(src.dtype), layout, outside_code(outside), _stream())
