"""ctypes binding of libatx_parcel — the ascent of one air parcel per column of a stack of temperature and specific humidity, on hybrid
model levels or on pressure levels: CAPE, CIN and the lifting condensation level (``include/atx_parcel.h``), a library of its own next
to libatx and the other vertical libraries.

There is no CPU fallback: if ``lib/libatx_parcel.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call raises.
Return codes map to the exception types of ``native``: ``ValueError``, ``AssertionError`` (shapes), ``NotImplementedError``.
"""

from __future__ import annotations

from ctypes import c_char_p, c_double, c_int, c_int64, c_void_p
from typing import Any

import torch

from ._binding import Library
from .native import EINVAL, ENOTIMPL, ESHAPE, OK, AtxError, _ptr, _stream, dtype_code  # noqa: F401 - OK is one of this module's names

HYBRID, PRESSURE = 0, 1  # atx_parcel_mode
LOWEST, MOST_UNSTABLE = 0, 1  # atx_parcel_start
PARCELS = {"lowest": LOWEST, "most-unstable": MOST_UNSTABLE}
OUTPUTS = ("cape", "cin", "plcl", "tlcl", "pstart")  # the rows of ``out``, ATX_PARCEL_OUTPUTS of them
MAX_LEVELS, BLOCK, NEWTON_STEPS = 256, 8, 10  # ATX_PARCEL_MAX_LEVELS, ATX_PARCEL_BLOCK, ATX_PARCEL_NEWTON_STEPS

# every symbol include/atx_parcel.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_parcel_version": (c_int, []),
    "atx_parcel_last_error": (c_char_p, []),
    "atx_parcel_columns": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_double, c_double,
         c_int, c_int, c_int, c_int, c_void_p],
    ),
    "atx_parcel_tile_points": (c_int, [c_int64, c_int, c_int, c_int]),
    "atx_parcel_host_math": (c_int, [c_void_p, c_void_p, c_int64, c_int]),
}

LIBRARY = Library("libatx_parcel.so", "ATX_PARCEL_LIBRARY", SIGNATURES, "atx_parcel_last_error",
                  errors={EINVAL: ValueError, ESHAPE: AssertionError, ENOTIMPL: NotImplementedError},
                  unmapped=lambda fn, message, code: AtxError(f"{fn}: {message} (code {code})"))
lib_path = LIBRARY.path  # ``lib/libatx_parcel.so`` next to this file; ``ATX_PARCEL_LIBRARY`` overrides it
load = LIBRARY.load  # opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def _call(fn: str, *args: Any) -> None:
    LIBRARY.check(fn, getattr(load(), fn)(*args))


def parcel_code(parcel) -> int:
    """``"lowest"`` / ``"most-unstable"`` (or the enum value itself) as ``atx_parcel_start``."""
    if isinstance(parcel, str):
        if parcel not in PARCELS:
            raise ValueError(f"unknown parcel {parcel!r}: one of {', '.join(PARCELS)}")
        return PARCELS[parcel]
    return int(parcel)


def tile_points(n_lev: int, dtype: torch.dtype, *, pressure_levels: bool, parcel="lowest") -> int:
    """The points of a tile of the column kernel for this shape (``atx_parcel_tile_points``); 0: one point does not fit."""
    return int(load().atx_parcel_tile_points(n_lev, dtype_code(dtype), PRESSURE if pressure_levels else HYBRID, parcel_code(parcel)))


def columns(t, q, sp, out, *, n_pts, n_lev, t_pitch, q_pitch, out_pitch, layout, A=None, B=None, levels_pa=None, parcel="lowest",
            depth_pa=30000.0, top_pa=5000.0) -> None:
    """The ascent of every point's parcel (``atx_parcel_columns``, include/atx_parcel.h holds the statement).  ``t`` / ``q`` / ``sp`` /
    ``out`` share a type and are device tensors, ``out`` of ``len(OUTPUTS)`` rows; ``A`` / ``B`` (``n_lev + 1`` half levels: hybrid levels)
    or ``levels_pa`` (``n_lev`` pressures: pressure levels) are float64 device tensors."""
    assert t.dtype == q.dtype == sp.dtype == out.dtype, (t.dtype, q.dtype, sp.dtype, out.dtype)
    assert sp.numel() == n_pts and sp.is_contiguous(), (sp.numel(), n_pts)
    if (levels_pa is None) == (A is None or B is None):
        raise ValueError("either A and B (hybrid levels) or levels_pa (pressure levels)")
    if levels_pa is None:
        assert A.dtype == B.dtype == torch.float64 and A.numel() == B.numel() == n_lev + 1, (A.dtype, A.numel(), B.numel(), n_lev)
    else:
        assert levels_pa.dtype == torch.float64 and levels_pa.numel() == n_lev, (levels_pa.dtype, levels_pa.numel(), n_lev)
    optional = lambda x: None if x is None else _ptr(x)  # noqa: E731
    _call("atx_parcel_columns", _ptr(t), _ptr(q), _ptr(sp), _ptr(out), optional(A), optional(B), optional(levels_pa), n_pts, n_lev, t_pitch, q_pitch,
          out_pitch, float(depth_pa), float(top_pa), dtype_code(t.dtype), layout, HYBRID if levels_pa is None else PRESSURE, parcel_code(parcel), _stream())
