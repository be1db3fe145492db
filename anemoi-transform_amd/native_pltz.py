"""ctypes binding of libatx_pltz — temperature and geopotential of a model-level column on pressure levels with the IFS extrapolations
under the ground, and mean sea level pressure: the hydrostatic integral, the bracket search, both interpolations, the extrapolations and
msl in one launch (``include/atx_pltz.h``), a library of its own next to libatx, libatx_levels, libatx_geopotential and libatx_heights.

There is no CPU fallback: if ``lib/libatx_pltz.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call raises.
Return codes map to the exception types of ``native``: ``ValueError``, ``AssertionError`` (shapes), ``NotImplementedError``.
"""

from __future__ import annotations

from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Any

import torch

from ._binding import Library
from .native import EINVAL, ENOTIMPL, ESHAPE, OK, AtxError, _ptr, _stream, dtype_code  # noqa: F401 - OK is one of this module's names

LINEAR, LOG = 0, 1  # atx_pltz_coordinate
COORDINATES = {"linear": LINEAR, "log": LOG}
MAX_LEVELS = 256  # ATX_PLTZ_MAX_LEVELS

# every symbol include/atx_pltz.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_pltz_version": (c_int, []),
    "atx_pltz_last_error": (c_char_p, []),
    "atx_pltz_interpolate": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
         c_int64, c_int, c_int, c_int, c_int, c_void_p],
    ),
}

LIBRARY = Library("libatx_pltz.so", "ATX_PLTZ_LIBRARY", SIGNATURES, "atx_pltz_last_error",
                  errors={EINVAL: ValueError, ESHAPE: AssertionError, ENOTIMPL: NotImplementedError},
                  unmapped=lambda fn, message, code: AtxError(f"{fn}: {message} (code {code})"))
lib_path = LIBRARY.path  # ``lib/libatx_pltz.so`` next to this file; ``ATX_PLTZ_LIBRARY`` overrides it
load = LIBRARY.load  # opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def _call(fn: str, *args: Any) -> None:
    LIBRARY.check(fn, getattr(load(), fn)(*args))


def coordinate_code(coordinate) -> int:
    """``"linear"`` / ``"log"`` (or the enum value itself) as ``atx_pltz_coordinate``."""
    if isinstance(coordinate, str):
        if coordinate not in COORDINATES:
            raise ValueError(f"unknown coordinate {coordinate!r}: one of {', '.join(COORDINATES)}")
        return COORDINATES[coordinate]
    return int(coordinate)


def interpolate(t, q, sp, zs, out, A, B, targets, *, n_pts, n_lev, n_tgt, t_pitch, q_pitch, out_pitch, layout, coordinate="linear", msl=True) -> None:
    """``t`` and ``q`` on ``n_lev`` model levels — the LOWEST ``n_lev`` of the ``A`` / ``B`` table — to ``out``: ``t`` at the ``n_tgt``
    pressures of ``targets`` (Pa), then ``z`` at them, then, with ``msl``, the mean sea level pressure, for every point
    (``atx_pltz_interpolate``, include/atx_pltz.h holds the statement).  ``t`` / ``q`` / ``sp`` / ``zs`` / ``out`` share a type; ``A`` /
    ``B`` / ``targets`` are float64 device tensors.  Every pointer is a device pointer."""
    assert t.dtype == q.dtype == sp.dtype == zs.dtype == out.dtype, (t.dtype, q.dtype, sp.dtype, zs.dtype, out.dtype)
    assert A.dtype == B.dtype == targets.dtype == torch.float64, (A.dtype, B.dtype, targets.dtype)
    assert A.numel() == B.numel() and targets.numel() == n_tgt
    assert sp.numel() == zs.numel() == n_pts and sp.is_contiguous() and zs.is_contiguous(), (sp.numel(), zs.numel())
    _call("atx_pltz_interpolate", _ptr(t), _ptr(q), _ptr(sp), _ptr(zs), _ptr(out), _ptr(A), _ptr(B), _ptr(targets), n_pts, n_lev, n_tgt, A.numel(),
          t_pitch, q_pitch, out_pitch, dtype_code(t.dtype), layout, coordinate_code(coordinate), int(bool(msl)), _stream())
