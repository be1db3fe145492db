"""ctypes binding of libatx_search — the first step of a column, read from either end, at which a search variable crosses a value, or the
level of its maximum or minimum, and the variables of a stack there (``include/atx_search.h``), a library of its own next to libatx and
the other vertical libraries.

There is no CPU fallback: if ``lib/libatx_search.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call raises.
Return codes map to the exception types of ``native``: ``ValueError``, ``AssertionError`` (shapes), ``NotImplementedError``.
"""

from __future__ import annotations

from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Any

import torch

from ._binding import Library
from .native import EINVAL, ENOTIMPL, ESHAPE, OK, AtxError, _ptr, _stream, dtype_code  # noqa: F401 - OK is one of this module's names

FORWARD, BACKWARD = 0, 1  # atx_search_direction
DIRECTIONS = {"forward": FORWARD, "backward": BACKWARD}
UP, DOWN, ANY, MAX, MIN = 0, 1, 2, 3, 4  # atx_search_mode
MODES = {"up": UP, "down": DOWN, "any": ANY, "max": MAX, "min": MIN}
MAX_LEVELS = 256  # ATX_SEARCH_MAX_LEVELS
ULPS_F64 = 11  # ATX_SEARCH_ULPS_F64

# every symbol include/atx_search.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_search_version": (c_int, []),
    "atx_search_last_error": (c_char_p, []),
    "atx_search_columns": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int,
         c_int, c_void_p],
    ),
}

LIBRARY = Library("libatx_search.so", "ATX_SEARCH_LIBRARY", SIGNATURES, "atx_search_last_error",
                  errors={EINVAL: ValueError, ESHAPE: AssertionError, ENOTIMPL: NotImplementedError},
                  unmapped=lambda fn, message, code: AtxError(f"{fn}: {message} (code {code})"))
lib_path = LIBRARY.path  # ``lib/libatx_search.so`` next to this file; ``ATX_SEARCH_LIBRARY`` overrides it
load = LIBRARY.load  # opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def _call(fn: str, *args: Any) -> None:
    LIBRARY.check(fn, getattr(load(), fn)(*args))


def _code(table: dict[str, int], what: str, value) -> int:
    if isinstance(value, str):
        if value not in table:
            raise ValueError(f"unknown {what} {value!r}: one of {', '.join(table)}")
        return table[value]
    return int(value)


def direction_code(direction) -> int:
    """``"forward"`` / ``"backward"`` (or the enum value itself) as ``atx_search_direction``."""
    return _code(DIRECTIONS, "direction", direction)


def mode_code(mode) -> int:
    """``"up"`` / ``"down"`` / ``"any"`` / ``"max"`` / ``"min"`` (or the enum value itself) as ``atx_search_mode``."""
    return _code(MODES, "mode", mode)


def columns(src, search, out, targets, *, n_pts, n_var, n_lev, n_tgt, src_pitch, search_pitch, out_pitch, layout, direction="forward", mode="any",
            level_values=None, count=None) -> None:
    """The first step of every point's ``search`` column, in scan order, that crosses ``targets[t]`` (or its extremum), and the ``n_var``
    variables of ``src`` — and ``level_values`` as one more — there (``atx_search_columns``, include/atx_search.h holds the statement).
    ``src`` / ``search`` / ``out`` share a type (``src`` is ``None`` where ``n_var == 0``, ``out`` where there is no output row);
    ``targets`` and ``level_values`` are float64 device tensors; ``count`` a uint8 device tensor of ``n_pts x n_tgt``.  Every pointer is a
    device pointer."""
    assert search.dtype == (search if src is None else src).dtype == (search if out is None else out).dtype, (search.dtype, src, out)
    if targets is not None:
        assert targets.dtype == torch.float64 and targets.numel() == n_tgt, (targets.dtype, targets.numel())
    if level_values is not None:
        assert level_values.dtype == torch.float64 and level_values.numel() == n_lev and level_values.is_contiguous(), (level_values.dtype, level_values.numel())
    if count is not None:
        assert count.dtype == torch.uint8 and count.numel() == n_pts * n_tgt and count.is_contiguous(), (count.dtype, count.numel())
    optional = lambda x: None if x is None else _ptr(x)  # noqa: E731
    _call("atx_search_columns", optional(src), _ptr(search), optional(out), optional(count), optional(targets), optional(level_values), n_pts, n_var,
          n_lev, n_tgt, src_pitch, search_pitch, out_pitch, dtype_code(search.dtype), layout, direction_code(direction), mode_code(mode), _stream())
