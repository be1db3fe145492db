"""ctypes binding of libatx_geopotential — the geopotential on model levels, integrated hydrostatically from the ground
(``include/atx_geopotential.h``), a library of its own next to libatx and libatx_levels.

There is no CPU fallback: if ``lib/libatx_geopotential.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call
raises.  Return codes map to the exception types of ``native``: ``ValueError``, ``AssertionError`` (shapes), ``NotImplementedError``.
"""

from __future__ import annotations

from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Any

import torch

from ._binding import Library
from .native import EINVAL, ENOTIMPL, ESHAPE, OK, AtxError, _ptr, _stream, dtype_code  # noqa: F401 - OK is one of this module's names

MAX_LEVELS = 256  # ATX_GEOPOTENTIAL_MAX_LEVELS

# every symbol include/atx_geopotential.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_geopotential_version": (c_int, []),
    "atx_geopotential_last_error": (c_char_p, []),
    "atx_geopotential_on_model_levels": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int,
         c_void_p],
    ),
}

LIBRARY = Library("libatx_geopotential.so", "ATX_GEOPOTENTIAL_LIBRARY", SIGNATURES, "atx_geopotential_last_error",
                  errors={EINVAL: ValueError, ESHAPE: AssertionError, ENOTIMPL: NotImplementedError},
                  unmapped=lambda fn, message, code: AtxError(f"{fn}: {message} (code {code})"))
lib_path = LIBRARY.path  # ``lib/libatx_geopotential.so`` next to this file; ``ATX_GEOPOTENTIAL_LIBRARY`` overrides it
load = LIBRARY.load  # opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def _call(fn: str, *args: Any) -> None:
    LIBRARY.check(fn, getattr(load(), fn)(*args))


def geopotential(t, q, sp, zs, A, B, out, *, n_pts, n_lev, t_pitch, q_pitch, out_pitch, layout) -> None:
    """The geopotential (m^2/s^2) of the ``n_lev`` LOWEST model levels of the ``A`` / ``B`` table for every point, integrated
    hydrostatically from the ground (``atx_geopotential_on_model_levels``, include/atx_geopotential.h holds the statement).  ``t`` / ``q`` /
    ``out`` / ``sp`` / ``zs`` share a type; ``zs`` is the surface geopotential or ``None`` (0.0 everywhere); ``A`` / ``B`` are float64
    device tensors.  Every pointer is a device pointer."""
    assert t.dtype == q.dtype == out.dtype == sp.dtype, (t.dtype, q.dtype, out.dtype, sp.dtype)
    assert A.dtype == B.dtype == torch.float64, (A.dtype, B.dtype)
    assert A.numel() == B.numel() and sp.numel() == n_pts and sp.is_contiguous()
    if zs is not None:
        assert zs.dtype == t.dtype and zs.numel() == n_pts and zs.is_contiguous(), (zs.dtype, zs.numel())
    _call("atx_geopotential_on_model_levels", _ptr(t), _ptr(q), _ptr(sp), None if zs is None else _ptr(zs), _ptr(A), _ptr(B), _ptr(out), n_pts,
          n_lev, A.numel(), t_pitch, q_pitch, out_pitch, dtype_code(t.dtype), layout, _stream())
