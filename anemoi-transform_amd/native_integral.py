"""ctypes binding of libatx_integral — pressure-weighted column integrals and layer means of the variables of a stack of levels, on
hybrid model levels or on pressure levels (``include/atx_integral.h``), a library of its own next to libatx and the other vertical
libraries.

There is no CPU fallback: if ``lib/libatx_integral.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call raises.
Return codes map to the exception types of ``native``: ``ValueError``, ``AssertionError`` (shapes), ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes
from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Any

import torch

from ._binding import Library
from .native import EINVAL, ENOTIMPL, ESHAPE, OK, AtxError, _ptr, _stream, dtype_code  # noqa: F401 - OK is one of this module's names

HYBRID, PRESSURE = 0, 1  # atx_integral_mode
SUM, MEAN = 0, 1  # atx_integral_kind
KINDS = {"integral": SUM, "mean": MEAN}
MAX_LEVELS, MAX_TERMS, MAX_BOUNDS = 256, 64, 32  # ATX_INTEGRAL_MAX_*
BLOCK = 8  # ATX_INTEGRAL_BLOCK
G = 9.80665  # ATX_INTEGRAL_G


def ulps_f64(n_lev: int, K: float) -> float:
    """``ATX_INTEGRAL_ULPS_F64``: the header's bound for a sum, in float64 ulps of sum |w f| / g; a mean has twice that."""
    return 16.0 * K + BLOCK + (n_lev + BLOCK - 1) // BLOCK + 2


# every symbol include/atx_integral.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_integral_version": (c_int, []),
    "atx_integral_last_error": (c_char_p, []),
    "atx_integral_columns": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
         c_int, c_int, c_int, c_int, c_void_p],
    ),
}

LIBRARY = Library("libatx_integral.so", "ATX_INTEGRAL_LIBRARY", SIGNATURES, "atx_integral_last_error",
                  errors={EINVAL: ValueError, ESHAPE: AssertionError, ENOTIMPL: NotImplementedError},
                  unmapped=lambda fn, message, code: AtxError(f"{fn}: {message} (code {code})"))
lib_path = LIBRARY.path  # ``lib/libatx_integral.so`` next to this file; ``ATX_INTEGRAL_LIBRARY`` overrides it
load = LIBRARY.load  # opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def _call(fn: str, *args: Any) -> None:
    LIBRARY.check(fn, getattr(load(), fn)(*args))


def kind_code(kind) -> int:
    """``"integral"`` / ``"mean"`` (or the enum value itself) as ``atx_integral_kind``."""
    if isinstance(kind, str):
        if kind not in KINDS:
            raise ValueError(f"unknown kind {kind!r}: one of {', '.join(KINDS)}")
        return KINDS[kind]
    return int(kind)


def columns(src, sp, out, terms, bounds, *, n_pts, n_var, n_lev, src_pitch, out_pitch, layout, A=None, B=None, levels_pa=None, kind="integral") -> None:
    """The ``len(terms)`` integrands of ``n_var`` variables of ``n_lev`` levels each, integrated over the ``len(bounds)`` layers of every
    point (``atx_integral_columns``, include/atx_integral.h holds the statement).  ``src`` / ``sp`` / ``out`` share a type and are device
    tensors; ``A`` / ``B`` (``n_lev + 1`` half levels: hybrid levels) or ``levels_pa`` (``n_lev`` pressures: pressure levels) are float64
    device tensors; ``terms`` — ``(v1, v2)`` pairs, ``v2 < 0`` for a single factor — and ``bounds`` — ``(top, bottom)`` in Pa — are HOST
    sequences."""
    assert src.dtype == sp.dtype == out.dtype, (src.dtype, sp.dtype, out.dtype)
    assert sp.numel() == n_pts and sp.is_contiguous(), (sp.numel(), n_pts)
    if (levels_pa is None) == (A is None or B is None):
        raise ValueError("either A and B (hybrid levels) or levels_pa (pressure levels)")
    if levels_pa is None:
        assert A.dtype == B.dtype == torch.float64 and A.numel() == B.numel() == n_lev + 1, (A.dtype, A.numel(), B.numel(), n_lev)
    else:
        assert levels_pa.dtype == torch.float64 and levels_pa.numel() == n_lev, (levels_pa.dtype, levels_pa.numel(), n_lev)
    flat_terms = [int(v) for term in terms for v in term]
    flat_bounds = [float(v) for bound in bounds for v in bound]
    n_term, n_bnd = len(flat_terms) // 2, len(flat_bounds) // 2
    optional = lambda x: None if x is None else _ptr(x)  # noqa: E731
    _call("atx_integral_columns", _ptr(src), _ptr(sp), _ptr(out), (ctypes.c_int32 * max(1, 2 * n_term))(*flat_terms),
          (ctypes.c_double * max(1, 2 * n_bnd))(*flat_bounds), optional(A), optional(B), optional(levels_pa), n_pts, n_var, n_lev, n_term, n_bnd,
          src_pitch, out_pitch, dtype_code(src.dtype), layout, HYBRID if levels_pa is None else PRESSURE, kind_code(kind), _stream())
