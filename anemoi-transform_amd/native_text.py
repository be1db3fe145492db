"""ctypes binding of libatx_text — the text-column kernels (``include/atx_text.h``), a library of its own next to libatx.

There is no CPU fallback: if ``lib/libatx_text.so`` is missing, or a tensor handed to the wrapper does not live in HBM, the call raises.
"""

from __future__ import annotations

from ctypes import c_char_p, c_int, c_int32, c_int64, c_void_p
from typing import Any

import torch

from ._binding import EINVAL, OK, Library  # noqa: F401 - the status codes are part of this module's names

MAX_WIDTH = 256  # ATX_TEXT_MAX_WIDTH

# every symbol include/atx_text.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_text_version": (c_int, []),
    "atx_text_last_error": (c_char_p, []),
    "atx_text_encode_statids": (c_int, [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p, c_void_p]),
}

LIBRARY = Library("libatx_text.so", "ATX_TEXT_LIBRARY", SIGNATURES, "atx_text_last_error")
lib_path = LIBRARY.path  # ``lib/libatx_text.so`` next to this file; ``ATX_TEXT_LIBRARY`` overrides it
load = LIBRARY.load  # libatx_text.so, opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def encode_statids(text: torch.Tensor, code: torch.Tensor, undecided: torch.Tensor) -> None:
    """``atx_text_encode_statids`` over the rows of ``text`` (uint8 ``[n, width]`` in HBM, rows contiguous, any row pitch) into ``code``
    (int64 ``[n]``) and ``undecided`` (uint8 ``[n]``), on the current stream."""
    if text.dim() != 2 or text.dtype != torch.uint8 or (text.shape[0] > 0 and text.shape[1] > 1 and text.stride(1) != 1) or \
            (text.shape[0] > 1 and text.stride(0) < text.shape[1]):  # a matrix of no rows has no strides to speak of
        raise ValueError(f"a text column is a uint8 [n, width] matrix with contiguous rows, got {text.dtype} {tuple(text.shape)} strides {text.stride()}")
    n, width = text.shape
    if code.dtype != torch.int64 or undecided.dtype != torch.uint8 or code.shape != (n,) or undecided.shape != (n,) or \
            not (code.is_contiguous() and undecided.is_contiguous()):
        raise ValueError(f"code must be a contiguous int64 [{n}] and undecided a contiguous uint8 [{n}]")
    for t in (text, code, undecided):
        if not t.is_cuda or t.device != text.device:
            raise ValueError("text, code and undecided must live in HBM on one device")
    handle = load()
    with torch.cuda.device(text.device):
        stream = torch.cuda.current_stream().cuda_stream
        status = handle.atx_text_encode_statids(text.data_ptr(), n, width, text.stride(0) if n > 1 else max(text.stride(0), width),
                                                code.data_ptr(), undecided.data_ptr(), stream)
    LIBRARY.check("atx_text_encode_statids", status)
