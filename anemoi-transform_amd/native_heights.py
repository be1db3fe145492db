"""ctypes binding of libatx_heights — the model levels of a stack of variables interpolated to geopotential heights above the ground or
above mean sea level, the hydrostatic integral, the bracket search and the interpolation in one launch (``include/atx_heights.h``), a
library of its own next to libatx, libatx_levels and libatx_geopotential.

There is no CPU fallback: if ``lib/libatx_heights.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call raises.
Return codes map to the exception types of ``native``: ``ValueError``, ``AssertionError`` (shapes), ``NotImplementedError``.
"""

from __future__ import annotations

from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Any

import torch

from ._binding import Library
from .native import EINVAL, ENOTIMPL, ESHAPE, OK, AtxError, _ptr, _stream, dtype_code  # noqa: F401 - OK is one of this module's names

ABOVE_GROUND, ABOVE_SEA = 0, 1  # atx_heights_reference
REFERENCES = {"ground": ABOVE_GROUND, "sea": ABOVE_SEA}
NEAREST, MISSING = 0, 1  # atx_heights_outside
OUTSIDE = {"nearest": NEAREST, "missing": MISSING}
MAX_LEVELS = 256  # ATX_HEIGHTS_MAX_LEVELS

# every symbol include/atx_heights.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_heights_version": (c_int, []),
    "atx_heights_last_error": (c_char_p, []),
    "atx_heights_interpolate": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64,
         c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, c_void_p],
    ),
}

LIBRARY = Library("libatx_heights.so", "ATX_HEIGHTS_LIBRARY", SIGNATURES, "atx_heights_last_error",
                  errors={EINVAL: ValueError, ESHAPE: AssertionError, ENOTIMPL: NotImplementedError},
                  unmapped=lambda fn, message, code: AtxError(f"{fn}: {message} (code {code})"))
lib_path = LIBRARY.path  # ``lib/libatx_heights.so`` next to this file; ``ATX_HEIGHTS_LIBRARY`` overrides it
load = LIBRARY.load  # opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def _call(fn: str, *args: Any) -> None:
    LIBRARY.check(fn, getattr(load(), fn)(*args))


def _code(value, table: dict[str, int], what: str) -> int:
    """A name of ``table`` (or the enum value itself) as the enum value."""
    if isinstance(value, str):
        if value not in table:
            raise ValueError(f"unknown {what} {value!r}: one of {', '.join(table)}")
        return table[value]
    return int(value)


def reference_code(reference) -> int:
    """``"ground"`` / ``"sea"`` (or the enum value itself) as ``atx_heights_reference``."""
    return _code(reference, REFERENCES, "reference")


def outside_code(outside) -> int:
    """``"nearest"`` / ``"missing"`` (or the enum value itself) as ``atx_heights_outside``."""
    return _code(outside, OUTSIDE, "outside policy")


def interpolate(src, out, t, q, sp, zs, A, B, targets, *, n_pts, n_var, n_lev, n_tgt, src_pitch, t_pitch, q_pitch, out_pitch, layout,
                reference="ground", outside="nearest") -> None:
    """``n_var`` variables of ``n_lev`` model levels each — the LOWEST ``n_lev`` of the ``A`` / ``B`` table — to the ``n_tgt``
    geopotentials of ``targets`` (m^2/s^2 above the ground, or above the sea) for every point (``atx_heights_interpolate``,
    include/atx_heights.h holds the statement).  ``src`` / ``out`` / ``t`` / ``q`` / ``sp`` / ``zs`` share a type; ``zs`` may be ``None``
    above the ground; ``A`` / ``B`` / ``targets`` are float64 device tensors.  Every pointer is a device pointer."""
    assert src.dtype == out.dtype == t.dtype == q.dtype == sp.dtype, (src.dtype, out.dtype, t.dtype, q.dtype, sp.dtype)
    assert A.dtype == B.dtype == targets.dtype == torch.float64, (A.dtype, B.dtype, targets.dtype)
    assert A.numel() == B.numel() and targets.numel() == n_tgt and sp.numel() == n_pts and sp.is_contiguous()
    if zs is not None:
        assert zs.dtype == src.dtype and zs.numel() == n_pts and zs.is_contiguous(), (zs.dtype, zs.numel())
    _call("atx_heights_interpolate", _ptr(src), _ptr(out), _ptr(t), _ptr(q), _ptr(sp), None if zs is None else _ptr(zs), _ptr(A), _ptr(B),
          _ptr(targets), n_pts, n_var, n_lev, n_tgt, A.numel(), src_pitch, t_pitch, q_pitch, out_pitch, dtype_code(src.dtype), layout,
          reference_code(reference), outside_code(outside), _stream())
