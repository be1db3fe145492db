"""ctypes binding of libatx_stat — the grid-box statistics over the rows of a CSR matrix: maximum, minimum, mode, variance and standard
deviation (``include/atx_stat.h``), a library of its own next to libatx.

There is no CPU fallback: if ``lib/libatx_stat.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call raises.
Return codes map to the exception types of ``native``: ``ValueError``, ``AssertionError`` (shapes), ``NotImplementedError``.
"""

from __future__ import annotations

from ctypes import c_char_p, c_double, c_int, c_int64, c_void_p
from typing import Any

import torch

from ._binding import Library
from .native import EINVAL, ENOTIMPL, ESHAPE, OK, AtxError, _ptr, _stream, dtype_code  # noqa: F401 - OK is one of this module's names

MAXIMUM, MINIMUM, MODE, VARIANCE, STDDEV = range(5)  # atx_statistic
STATISTICS = {"maximum": MAXIMUM, "minimum": MINIMUM, "mode": MODE, "variance": VARIANCE, "standard-deviation": STDDEV}
UNWEIGHTED = (MAXIMUM, MINIMUM)  # the statistics that are defined without weights (data = None)
MISSING_ANY, MISSING_ALL, MISSING_HEAVIEST = 0, 1, 2  # atx_stat_missing
MISSING_POLICIES = {None: MISSING_ANY, "all": MISSING_ALL, "heaviest": MISSING_HEAVIEST}

# every symbol include/atx_stat.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_stat_version": (c_int, []),
    "atx_stat_last_error": (c_char_p, []),
    "atx_regrid_csr_stat": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int,
         c_double, c_void_p],
    ),
}

LIBRARY = Library("libatx_stat.so", "ATX_STAT_LIBRARY", SIGNATURES, "atx_stat_last_error",
                  errors={EINVAL: ValueError, ESHAPE: AssertionError, ENOTIMPL: NotImplementedError},
                  unmapped=lambda fn, message, code: AtxError(f"{fn}: {message} (code {code})"))
lib_path = LIBRARY.path  # ``lib/libatx_stat.so`` next to this file; ``ATX_STAT_LIBRARY`` overrides it
load = LIBRARY.load  # libatx_stat.so, opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def _call(fn: str, *args: Any) -> None:
    LIBRARY.check(fn, getattr(load(), fn)(*args))


def statistic_code(statistic) -> int:
    """``"maximum"`` / ``"minimum"`` / ``"mode"`` / ``"variance"`` / ``"standard-deviation"`` (or the enum value itself) as ``atx_statistic``."""
    if isinstance(statistic, str):
        if statistic not in STATISTICS:
            raise ValueError(f"unknown statistic {statistic!r}: one of {', '.join(STATISTICS)}")
        return STATISTICS[statistic]
    return int(statistic)


def missing_policy_code(policy) -> int:
    """``None`` (a missing source makes its target missing) / ``"all"`` / ``"heaviest"`` (or the enum value itself) as ``atx_stat_missing``."""
    if policy is None or isinstance(policy, str):
        if policy not in MISSING_POLICIES:
            raise ValueError(f"unknown missing-value policy {policy!r}: one of None, 'all', 'heaviest'")
        return MISSING_POLICIES[policy]
    return int(policy)


def regrid_csr_stat(src, out, indptr, indices, data, *, n_src, n_tgt, nnz, n_lev, src_pitch, out_pitch, layout, statistic, policy=None,
                    min_valid: float = 0.0) -> None:
    """The statistic of the sources that row t of a CSR matrix names, for every target and level (``atx_regrid_csr_stat``,
    include/atx_stat.h holds the statement).  ``data`` — the shares — may be ``None`` for the maximum and the minimum: every entry then
    weighs 1.  ``policy``: ``None`` (NaN as soon as one source is), ``"all"`` (only when every source is) or ``"heaviest"`` (also when
    the first heaviest entry is); ``min_valid``: the share of the row's weight that must be valid.  Column stacks."""
    assert src.dtype == out.dtype, (src.dtype, out.dtype)
    if data is not None:
        assert data.dtype == src.dtype, (data.dtype, src.dtype)
    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32
    _call("atx_regrid_csr_stat", _ptr(src), _ptr(out), _ptr(indptr), _ptr(indices), _ptr(data), n_src, n_tgt, nnz, n_lev, src_pitch, out_pitch,
          dtype_code(src.dtype), layout, statistic_code(statistic), missing_policy_code(policy), float(min_valid), _stream())
