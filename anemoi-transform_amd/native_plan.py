"""ctypes binding of libatx_plan — the plan-time kernels (``include/atx_plan.h``), a library of its own next to libatx.

There is no CPU fallback: if ``lib/libatx_plan.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call raises.
"""

from __future__ import annotations

from ctypes import c_char_p, c_int, c_int64, c_void_p
from typing import Any

import torch

from ._binding import EINVAL, OK, Library  # noqa: F401 - the status codes are part of this module's names

_TABLES = [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64]  # zs .. n_src, zt .. n_tgt

# every symbol include/atx_plan.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_plan_version": (c_int, []),
    "atx_plan_last_error": (c_char_p, []),
    "atx_plan_box_average_count": (c_int, [*_TABLES, c_void_p, c_void_p]),
    "atx_plan_box_average_fill": (c_int, [*_TABLES, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
}

LIBRARY = Library("libatx_plan.so", "ATX_PLAN_LIBRARY", SIGNATURES, "atx_plan_last_error")
lib_path = LIBRARY.path  # ``lib/libatx_plan.so`` next to this file; ``ATX_PLAN_LIBRARY`` overrides it
load = LIBRARY.load  # libatx_plan.so, opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


class RowTable:
    """A row table in HBM (``include/atx_plan.h``): ``z`` float64 ``[rows + 1]``, ``len`` int64 ``[rows]``, ``start`` int64 ``[rows + 1]``."""

    def __init__(self, z: torch.Tensor, length: torch.Tensor, start: torch.Tensor, n_points: int) -> None:
        rows = length.shape[0] if length.dim() == 1 else -1
        for name, t, dtype, size in (("z", z, torch.float64, rows + 1), ("len", length, torch.int64, rows), ("start", start, torch.int64, rows + 1)):
            if t.dtype != dtype or t.shape != (size,) or not t.is_contiguous() or not t.is_cuda or t.device != z.device:
                raise ValueError(f"row table: {name} must be a contiguous {dtype} [{size}] in HBM on one device, got {t.dtype} "
                                 f"{tuple(t.shape)} on {t.device}")
        if rows < 1:
            raise ValueError("a row table has at least one row")
        self.z, self.len, self.start, self.rows, self.n_points = z, length, start, rows, int(n_points)

    def args(self) -> tuple:
        return self.z.data_ptr(), self.len.data_ptr(), self.start.data_ptr(), self.rows, self.n_points


def box_average_count(src: RowTable, tgt: RowTable, count: torch.Tensor) -> None:
    """``atx_plan_box_average_count``: the number of entries of every target cell into ``count`` (int64 ``[n_tgt]``), on the current stream."""
    if count.dtype != torch.int64 or count.shape != (tgt.n_points,) or not count.is_contiguous() or count.device != tgt.z.device or \
            src.z.device != tgt.z.device:
        raise ValueError(f"count must be a contiguous int64 [{tgt.n_points}] on the device of the row tables")
    handle = load()
    with torch.cuda.device(count.device):
        stream = torch.cuda.current_stream().cuda_stream
        LIBRARY.check("atx_plan_box_average_count", handle.atx_plan_box_average_count(*src.args(), *tgt.args(), count.data_ptr(), stream))


def box_average_fill(src: RowTable, tgt: RowTable, indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor) -> None:
    """``atx_plan_box_average_fill``: ``indices`` (int32 ``[nnz]``) and ``data`` (float64 ``[nnz]``) of the rows that ``indptr``
    (int32 ``[n_tgt + 1]``, the scan of the counts) lays out, on the current stream."""
    nnz = indices.shape[0] if indices.dim() == 1 else -1
    if indptr.dtype != torch.int32 or indptr.shape != (tgt.n_points + 1,) or indices.dtype != torch.int32 or nnz < 0 or \
            data.dtype != torch.float64 or data.shape != (nnz,) or not (indptr.is_contiguous() and indices.is_contiguous() and data.is_contiguous()):
        raise ValueError(f"indptr must be a contiguous int32 [{tgt.n_points + 1}], indices int32 [nnz] and data float64 [nnz]")
    for t in (indptr, indices, data, src.z):
        if t.device != tgt.z.device:
            raise ValueError("the row tables, indptr, indices and data must live in HBM on one device")
    handle = load()
    with torch.cuda.device(indptr.device):
        stream = torch.cuda.current_stream().cuda_stream
        LIBRARY.check("atx_plan_box_average_fill", handle.atx_plan_box_average_fill(
            *src.args(), *tgt.args(), indptr.data_ptr(), nnz, indices.data_ptr(), data.data_ptr(), stream))
