"""ctypes binding of libatx_missing — the weighted gather that drops NaN sources and renormalises (``include/atx_missing.h``), a
library of its own next to libatx.

There is no CPU fallback: if ``lib/libatx_missing.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call raises.
Return codes map to the exception types of ``native``: ``ValueError``, ``AssertionError`` (shapes), ``NotImplementedError``.
"""

from __future__ import annotations

from ctypes import c_char_p, c_double, c_int, c_int32, c_int64, c_void_p
from typing import Any

import torch

from ._binding import Library
from .native import EINVAL, ELL_PADDED, ENOTIMPL, ESHAPE, OK, AtxError, _ptr, _stream, dtype_code  # noqa: F401 - OK is one of this module's names

MISSING_ALL, MISSING_HEAVIEST = 0, 1  # atx_missing_policy
MISSING_POLICIES = {"all": MISSING_ALL, "heaviest": MISSING_HEAVIEST}

# every symbol include/atx_missing.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_missing_version": (c_int, []),
    "atx_missing_last_error": (c_char_p, []),
    "atx_regrid_ell_missing": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int64, c_int64, c_int64, c_int, c_int, c_int32, c_int, c_double,
         c_void_p],
    ),
    "atx_regrid_csr_missing": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_double,
         c_void_p],
    ),
}

LIBRARY = Library("libatx_missing.so", "ATX_MISSING_LIBRARY", SIGNATURES, "atx_missing_last_error",
                  errors={EINVAL: ValueError, ESHAPE: AssertionError, ENOTIMPL: NotImplementedError},
                  unmapped=lambda fn, message, code: AtxError(f"{fn}: {message} (code {code})"))
lib_path = LIBRARY.path  # ``lib/libatx_missing.so`` next to this file; ``ATX_MISSING_LIBRARY`` overrides it
load = LIBRARY.load  # libatx_missing.so, opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def _call(fn: str, *args: Any) -> None:
    LIBRARY.check(fn, getattr(load(), fn)(*args))


def missing_policy_code(policy) -> int:
    """``"all"`` / ``"heaviest"`` (or the enum value itself) as ``atx_missing_policy``."""
    if isinstance(policy, str):
        if policy not in MISSING_POLICIES:
            raise ValueError(f"unknown missing-value policy {policy!r}: one of {sorted(MISSING_POLICIES)}")
        return MISSING_POLICIES[policy]
    return int(policy)


def regrid_ell_missing(src, out, idx, w, *, n_src, n_tgt, k, n_lev, src_pitch, out_pitch, layout, policy, min_valid: float = 0.0,
                       padded: bool = False) -> None:
    """``native.regrid_ell`` that drops NaN sources and renormalises over the valid ones (``atx_regrid_ell_missing``,
    include/atx_missing.h holds the statement): ``policy`` ``"all"`` (NaN only when every source is) or ``"heaviest"`` (also when the first
    heaviest entry is); ``min_valid``: the share of the row's weight that must be valid.  Column stacks; weights are required."""
    assert src.dtype == out.dtype, (src.dtype, out.dtype)
    assert idx.dtype == torch.int32
    if w is not None:
        assert w.dtype == src.dtype, (w.dtype, src.dtype)
    _call("atx_regrid_ell_missing", _ptr(src), _ptr(out), _ptr(idx), _ptr(w), n_src, n_tgt, k, n_lev, src_pitch, out_pitch,
          dtype_code(src.dtype), layout, ELL_PADDED if padded else 0, missing_policy_code(policy), float(min_valid), _stream())


def regrid_csr_missing(src, out, indptr, indices, data, *, n_src, n_tgt, nnz, n_lev, src_pitch, out_pitch, layout, policy,
                       min_valid: float = 0.0) -> None:
    """``native.regrid_csr`` with the missing-value statement of ``regrid_ell_missing`` (``atx_regrid_csr_missing``)."""
    assert src.dtype == out.dtype == data.dtype, (src.dtype, out.dtype, data.dtype)
    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32
    _call("atx_regrid_csr_missing", _ptr(src), _ptr(out), _ptr(indptr), _ptr(indices), _ptr(data), n_src, n_tgt, nnz, n_lev, src_pitch,
          out_pitch, dtype_code(src.dtype), layout, missing_policy_code(policy), float(min_valid), _stream())
