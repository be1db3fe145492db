"""ctypes binding of libatx — the only compute path of this package.

There is no CPU fallback: if ``lib/libatx.so`` is missing, or a tensor handed to
one of the wrappers does not live in HBM, the call raises.  Return codes of the
C ABI (``include/atx.h``) are mapped to the exception types the reference raises
on this path: ``ValueError`` for bad configuration, ``AssertionError`` for shape
mismatches (R: filters/fields/regrid.py:377-378), ``NotImplementedError`` for
unsupported combinations (R: regrid.py:332-335).
"""

from __future__ import annotations

import ctypes
import os
import threading
from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p
from typing import Any

import numpy as np
import torch

from ._binding import Library

# atx_dtype / atx_layout / atx_cmp / atx_op / atx_red (include/atx.h)
F32, F64 = 0, 1
COLUMNS, FIELDS = 0, 1
CMP_GT, CMP_LT, CMP_EQ, CMP_NE, CMP_GE, CMP_LE, CMP_NOTNAN, CMP_ISNAN = range(8)
(
    OP_COPY,
    OP_AFFINE,
    OP_AFFINE_INV,
    OP_MUL,
    OP_DIV,
    OP_CLIP,
    OP_IMPUTE_NAN,
    OP_EXP,
    OP_LOG,
    OP_SET_NAN,
) = range(10)
RED_MIN, RED_MAX, RED_NANCOUNT, RED_MINMAX = range(4)
(COMB_SNOW_DEPTH_M, COMB_SNOW_COVER, COMB_COS_SIN, COMB_ATAN2, COMB_W_TO_WZ, COMB_WZ_TO_W, COMB_SUM, COMB_SUB, COMB_XY_TO_POLAR,
 COMB_POLAR_TO_XY, COMB_OPERA_CLIP, COMB_OPERA_PREPROCESS, COMB_ORAS6, COMB_LOOKUP, COMB_R_TO_D, COMB_D_TO_R, COMB_Q_TO_R,
 COMB_R_TO_Q, COMB_Q_TO_D, COMB_D_TO_Q) = range(20)
# what a level of a COMB_ORAS6 stack holds (ATX_ORAS6_* of atx.h)
ORAS6_KEEP, ORAS6_ZERO, ORAS6_TEMPERATURE, ORAS6_CELSIUS, ORAS6_HEAT, ORAS6_SURFACE = range(6)
COMB_DEGREES = 1
COMB_MAX_INPUTS = 8
FRAME_ROTATION, FRAME_GENERAL = 0, 1  # atx_frame: the kind of an atx_rotate_vectors_stack table (2 or 4 words per point)

OK, EINVAL, ESHAPE, ENOTIMPL, EHIP, EALIGN, EWORKSPACE, ECOMM = 0, -1, -2, -3, -4, -5, -6, -7
COMM_ID_BYTES = 128

# numpy layout of `atx_level_op` (24 bytes)
LEVEL_OP_DTYPE = np.dtype([("op", "<i4"), ("use_mask", "<i4"), ("p0", "<f8"), ("p1", "<f8")])

# every symbol include/atx.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_version": (c_int, []),
    "atx_last_error": (c_char_p, []),
    "atx_strerror": (c_char_p, [c_int]),
    "atx_last_route": (c_char_p, []),
    "atx_last_gather_route": (c_char_p, []),
    "atx_device_count": (c_int, []),
    "atx_set_tuning": (c_int, [c_int]),
    "atx_regrid_ell": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int64, c_int64, c_int64, c_int, c_int, c_int32,
         c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p],
    ),
    "atx_regrid_ell_batch": (
        c_int,
        [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int64, c_int64, c_int64, c_int, c_int,
         c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p],
    ),
    "atx_regrid_ell_ordered": (
        c_int,
        [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int64, c_int64, c_int64, c_int, c_int, c_int32,
         c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p],
    ),
    "atx_regrid_csr": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int,
         c_int, c_void_p, c_int32, c_void_p, c_void_p],
    ),
    "atx_regrid_csr_ordered": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int,
         c_int, c_void_p, c_int32, c_void_p, c_void_p],
    ),
    "atx_check_indices": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "atx_pointwise_stack": (
        c_int,
        [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p],
    ),
    "atx_combine_stack": (
        c_int,
        [c_int, POINTER(c_void_p), c_int32, POINTER(c_void_p), c_int32, c_int64, c_int64, c_int64, c_int, c_int, c_void_p,
         c_int32, c_void_p],
    ),
    "atx_pressure_at_height_stack": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_double, c_void_p, c_void_p],
    ),
    "atx_rotate_vectors_stack": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_int, c_void_p],
    ),
    "atx_obs_best_per_cell": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int64, c_void_p, c_int32, c_int64, c_int64, c_int64, c_int, c_int, c_int64,
         c_double, c_void_p, c_void_p, c_void_p],
    ),
    "atx_obs_fill_stack": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int64, c_int32, c_int64, c_void_p, c_int64, c_int, c_void_p]),
    "atx_obs_group_mean": (
        c_int, [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p],
    ),
    "atx_obs_group_argmin": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "atx_obs_forcings": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_uint32, c_void_p, c_int64, c_void_p]),
    "atx_obs_view_angles": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_uint32, c_void_p, c_int64, c_void_p]),
    "atx_obs_planck_bt": (c_int, [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "atx_healpix_ang2pix": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "atx_obs_fill_heights": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p,
         c_void_p, c_void_p, c_void_p],
    ),
    "atx_obs_column_ops": (c_int, [c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_void_p), POINTER(c_void_p), c_int64, c_void_p]),
    "atx_obs_row_expr": (
        c_int,
        [c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), c_int32, POINTER(c_void_p), c_int32, POINTER(c_double), c_int32,
         POINTER(c_void_p), c_int, c_void_p, c_void_p, c_int64, c_void_p],
    ),
    "atx_obs_keep_positions": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "atx_obs_order_key": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "atx_obs_mark_first": (c_int, [c_int32, POINTER(c_void_p), c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "atx_obs_take_rows": (
        c_int, [c_int32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int32), c_void_p, c_int64, c_int64, c_void_p, c_void_p],
    ),
    "atx_mask_build": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_double, c_int, c_void_p]),
    "atx_mask_count": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "atx_mask_to_index_workspace": (c_size_t, [c_int64]),
    "atx_mask_to_index": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "atx_knn_workspace_bytes": (c_size_t, [c_int64]),
    "atx_knn_build": (c_int, [c_void_p, c_int64, c_void_p, c_size_t, c_void_p]),
    "atx_knn_query": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "atx_cutout_inside": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p]),
    "atx_stream_copy": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "atx_vector_program": (c_int64, [c_void_p, c_int32, c_int64, c_int, c_void_p, c_int64]),
    "atx_reduce_workspace": (c_size_t, []),
    "atx_reduce": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "atx_relayout": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_void_p]),
    "atx_reduce_stack": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "atx_select_levels": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_void_p]),
    "atx_comm_version": (c_int, []),
    "atx_comm_unique_id": (c_int, [c_void_p]),
    "atx_comm_init": (c_int, [POINTER(c_void_p), c_int32, c_int32, c_void_p]),
    "atx_comm_destroy": (c_int, [c_void_p]),
    "atx_comm_rank": (c_int, [c_void_p]),
    "atx_comm_world": (c_int, [c_void_p]),
    "atx_bcast": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "atx_all_gather": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "atx_exchange": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64), POINTER(c_void_p), POINTER(c_int64), c_void_p]),
    "atx_gather_shards": (c_int, [c_void_p, c_void_p, POINTER(c_int64), c_void_p]),
}

class AtxError(RuntimeError):
    """HIP runtime failure inside libatx."""


def _failure(fn: str, message: str, code: int) -> AtxError:
    return AtxError(f"{fn}: {message}" if code == ECOMM else f"{fn}: {message} (code {code})")


LIBRARY = Library("libatx.so", "ATX_LIBRARY", SIGNATURES, "atx_last_error", strerror="atx_strerror", unmapped=_failure,
                  errors={EINVAL: ValueError, ESHAPE: AssertionError, ENOTIMPL: NotImplementedError})
lib_path = LIBRARY.path  # ``lib/libatx.so`` next to this file; ``ATX_LIBRARY`` overrides it (A/B builds of the kernels)
load = LIBRARY.load
# a build of libatx.so opened apart from load()'s and swapped in: side-by-side timing of two builds in one process (tools/kernel_bench.py --lib)
open_library = LIBRARY.open
use_library = LIBRARY.use


def _call(fn: str, *args: Any) -> None:
    code = getattr(load(), fn)(*args)
    if code != OK:
        LIBRARY.check(fn, code)


def _ptr(t: torch.Tensor | None) -> int | None:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"libatx works on HBM-resident tensors only, got a {t.device} tensor (no CPU fallback)")
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def dtype_code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return F32
    if dtype == torch.float64:
        return F64
    raise ValueError(f"libatx supports float32 / float64 stacks, got {dtype}")


def version() -> int:
    return load().atx_version()


def device_count() -> int:
    return load().atx_device_count()


def set_tuning(tile: int) -> None:
    _call("atx_set_tuning", int(tile))


# --------------------------------------------------------------------------------
# tensor-level wrappers (these are what the filters call)
# --------------------------------------------------------------------------------
ELL_PADDED = 1


def _program_companions(prog, dtype) -> tuple[int | None, int | None]:
    """``(vec_prog device pointer, host_prog host pointer)`` that ``level_program`` attached to a program tensor, if any."""
    if prog is None:
        return None, None
    vec = getattr(prog, "vec_prog", {}).get(dtype)
    host = getattr(prog, "host_prog", None)
    return _ptr(vec), (None if host is None else host.ctypes.data)


def regrid_ell(src, out, idx, w, *, n_src, n_tgt, k, n_lev, src_pitch, out_pitch, layout, prog=None, n_stage=0,
               tgt_mask=None, padded: bool = False, tgt_rows=None) -> None:
    """out[t, l] = sum_j w[t, j] * src[idx[t, j], l]; ``w is None`` -> pure k = 1 gather;
    ``padded``: negative indices are absent entries of padded ragged rows (ATX_ELL_PADDED);
    ``tgt_rows`` (device int32 permutation): ordered traversal — table row t is output row ``tgt_rows[t]``
    (``atx_regrid_ell_ordered``; column stacks only)."""
    if tgt_rows is not None:
        return regrid_ell_batch([src], [out], idx, w, n_src=n_src, n_tgt=n_tgt, k=k, n_lev=n_lev, src_pitch=src_pitch, out_pitch=out_pitch,
                                layout=layout, prog=prog, n_stage=n_stage, tgt_mask=tgt_mask, padded=padded, tgt_rows=tgt_rows)
    _call("atx_regrid_ell", *_regrid_ell_args(src, out, idx, w, n_src, n_tgt, k, n_lev, src_pitch, out_pitch, layout, prog, n_stage, tgt_mask,
                                              padded), _stream())


def _regrid_ell_args(src, out, idx, w, n_src, n_tgt, k, n_lev, src_pitch, out_pitch, layout, prog, n_stage, tgt_mask, padded) -> tuple:
    """The arguments of ``atx_regrid_ell`` up to (not including) the stream, checked and converted."""
    assert src.dtype == out.dtype, (src.dtype, out.dtype)
    assert idx.dtype == torch.int32
    if w is not None:
        assert w.dtype == src.dtype, (w.dtype, src.dtype)
    vec, host = _program_companions(prog, src.dtype)
    return (_ptr(src), _ptr(out), _ptr(idx), _ptr(w), n_src, n_tgt, k, n_lev, src_pitch, out_pitch, dtype_code(src.dtype), layout,
            ELL_PADDED if padded else 0, _ptr(prog), vec, host, n_stage, _ptr(tgt_mask))


class BoundCall:
    """One libatx entry point with its arguments checked and converted ONCE, for call sites that repeat the same launch on the same
    buffers (a one-field regrid per time step is launch-bound: its kernel runs 3 us, the Python marshalling of 19 arguments costs
    more than that).  ``__call__`` enqueues on the stream that was current when the call was bound, or on ``stream=`` given then.
    The object keeps the tensors it points into alive."""

    __slots__ = ("_fn", "_name", "_args", "_keep")

    def __init__(self, name: str, args: tuple, keep: tuple, stream: int | None = None) -> None:
        self._fn = getattr(load(), name)
        self._name = name
        self._args = (*args, _stream() if stream is None else stream)
        self._keep = keep

    def __call__(self) -> None:
        code = self._fn(*self._args)
        if code != OK:
            LIBRARY.check(self._name, code)


def bind_regrid_ell(src, out, idx, w, *, n_src, n_tgt, k, n_lev, src_pitch, out_pitch, layout, prog=None, n_stage=0, tgt_mask=None,
                    padded: bool = False, stream: int | None = None) -> BoundCall:
    """``regrid_ell`` (natural target order) as a ``BoundCall``."""
    args = _regrid_ell_args(src, out, idx, w, n_src, n_tgt, k, n_lev, src_pitch, out_pitch, layout, prog, n_stage, tgt_mask, padded)
    return BoundCall("atx_regrid_ell", args, (src, out, idx, w, prog, tgt_mask), stream)


def regrid_ell_batch(srcs, outs, idx, w, *, n_src, n_tgt, k, n_lev, src_pitch, out_pitch, layout, prog=None, n_stage=0,
                     tgt_mask=None, padded: bool = False, tgt_rows=None) -> None:
    """``regrid_ell`` over several stacks of identical shape in one launch (``atx_regrid_ell_batch``; with ``tgt_rows``:
    ``atx_regrid_ell_ordered``): ``srcs`` / ``outs`` are sequences of device tensors."""
    assert len(srcs) == len(outs) >= 1
    assert idx.dtype == torch.int32
    dtype = srcs[0].dtype
    assert all(t.dtype == dtype for t in srcs) and all(t.dtype == dtype for t in outs) and (w is None or w.dtype == dtype)
    n = len(srcs)
    src_ptrs = (c_void_p * n)(*[_ptr(t) for t in srcs])
    out_ptrs = (c_void_p * n)(*[_ptr(t) for t in outs])
    vec, host = _program_companions(prog, dtype)
    if tgt_rows is not None:
        assert tgt_rows.dtype == torch.int32 and tgt_rows.numel() >= n_tgt
        _call(
            "atx_regrid_ell_ordered", ctypes.cast(src_ptrs, c_void_p), ctypes.cast(out_ptrs, c_void_p), n, _ptr(idx), _ptr(w), _ptr(tgt_rows),
            n_src, n_tgt, k, n_lev, src_pitch, out_pitch, dtype_code(dtype), layout, ELL_PADDED if padded else 0, _ptr(prog), vec, host,
            n_stage, _ptr(tgt_mask), _stream(),
        )
        return
    _call(
        "atx_regrid_ell_batch", ctypes.cast(src_ptrs, c_void_p), ctypes.cast(out_ptrs, c_void_p), n, _ptr(idx), _ptr(w), n_src,
        n_tgt, k, n_lev, src_pitch, out_pitch, dtype_code(dtype), layout, ELL_PADDED if padded else 0, _ptr(prog), vec, host, n_stage,
        _ptr(tgt_mask), _stream(),
    )


def regrid_csr(src, out, indptr, indices, data, *, n_src, n_tgt, nnz, n_lev, src_pitch, out_pitch, layout, prog=None,
               n_stage=0, tgt_mask=None, tgt_rows=None) -> None:
    """out[t, l] = sum over the CSR row t of data * src[indices, l] (scipy csr_matvec order); with ``tgt_rows`` (device int32
    permutation) CSR row t is output row ``tgt_rows[t]`` (``atx_regrid_csr_ordered``; column stacks only)."""
    assert src.dtype == out.dtype == data.dtype, (src.dtype, out.dtype, data.dtype)
    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32
    if tgt_rows is not None:
        assert tgt_rows.dtype == torch.int32 and tgt_rows.numel() >= n_tgt
        _call(
            "atx_regrid_csr_ordered", _ptr(src), _ptr(out), _ptr(indptr), _ptr(indices), _ptr(data), _ptr(tgt_rows), n_src, n_tgt, nnz, n_lev,
            src_pitch, out_pitch, dtype_code(src.dtype), layout, _ptr(prog), n_stage, _ptr(tgt_mask), _stream(),
        )
        return
    _call(
        "atx_regrid_csr", _ptr(src), _ptr(out), _ptr(indptr), _ptr(indices), _ptr(data), n_src, n_tgt, nnz, n_lev,
        src_pitch, out_pitch, dtype_code(src.dtype), layout, _ptr(prog), n_stage, _ptr(tgt_mask), _stream(),
    )


def check_indices(idx, n_src: int) -> int:
    """Number of entries of ``idx`` outside [0, n_src) (synchronises)."""
    n_bad = torch.zeros(1, dtype=torch.int64, device=idx.device)
    _call("atx_check_indices", _ptr(idx), idx.numel(), n_src, _ptr(n_bad), _stream())
    return int(n_bad.item())


_PROGRAM_CACHE: dict[Any, torch.Tensor] = {}
_PROGRAM_CACHE_SIZE = 64


def level_program(stages: list[list[tuple[int, int, float, float]]], device, cache: bool = False) -> torch.Tensor:
    """Device copy of a per-level program: ``stages[s][l] = (op, use_mask, p0, p1)``.

    ``cache=True`` (the filters' call): programs are remembered by value — a pipeline applies the same program to every
    FieldList of a job, and rebuilding it (three small host-to-device copies and the per-vector tables) costs about as
    much host time as the launch it drives.  Cached programs are shared: treat them as read-only."""
    key = None
    if cache:
        key = (tuple(tuple(tuple(entry) for entry in stage) for stage in stages), str(device))
        hit = _PROGRAM_CACHE.get(key)
        if hit is not None:
            return hit
    raw = _build_level_program(stages, device)
    if key is not None:
        if len(_PROGRAM_CACHE) >= _PROGRAM_CACHE_SIZE:
            _PROGRAM_CACHE.pop(next(iter(_PROGRAM_CACHE)))
        _PROGRAM_CACHE[key] = raw
    return raw


def _build_level_program(stages, device) -> torch.Tensor:
    n_stage = len(stages)
    n_lev = len(stages[0])
    host = np.zeros(n_stage * n_lev, dtype=LEVEL_OP_DTYPE)
    for s, stage in enumerate(stages):
        assert len(stage) == n_lev
        for l, (op, use_mask, p0, p1) in enumerate(stage):
            host[s * n_lev + l] = (op, use_mask, p0, p1)
    raw = torch.from_numpy(host.view(np.uint8).copy()).to(device)
    # the host copy and the per-vector forms (atx_vector_program, host side) ride along: kernels given them need no
    # per-workgroup set-up (atx_regrid_ell: host_prog / vec_prog; atx_pointwise_stack: vec_prog)
    raw.host_prog = host
    raw.vec_prog = {}
    if raw.is_cuda:
        lib = load()
        for tdtype, code in ((torch.float32, F32), (torch.float64, F64)):
            n_entries = lib.atx_vector_program(host.ctypes.data, n_stage, n_lev, code, None, 0)
            table = np.zeros(n_entries, dtype=LEVEL_OP_DTYPE)
            got = lib.atx_vector_program(host.ctypes.data, n_stage, n_lev, code, table.ctypes.data, n_entries)
            if got != n_entries:
                raise AtxError(f"atx_vector_program: {lib.atx_last_error().decode()}")
            raw.vec_prog[tdtype] = torch.from_numpy(table.view(np.uint8).copy()).to(device)
    return raw


def pointwise_stack(x, y, *, n_pts, n_lev, x_pitch, y_pitch, layout, prog, n_stage, point_mask=None) -> None:
    assert x.dtype == y.dtype
    vec, host = _program_companions(prog, x.dtype)
    _call(
        "atx_pointwise_stack", _ptr(x), _ptr(y), n_pts, n_lev, x_pitch, y_pitch, dtype_code(x.dtype), layout,
        _ptr(prog), vec, host, n_stage, _ptr(point_mask), _stream(),
    )


def last_route() -> str:
    """The launch form this thread's last ``pointwise_stack`` took (``atx_last_route``: a diagnostic, ``"none"`` when it launched nothing)."""
    return load().atx_last_route().decode()


def last_gather_route() -> str:
    """The launch form this thread's last ``regrid_ell`` / ``regrid_ell_batch`` / ``regrid_csr`` took (``atx_last_gather_route``: a
    diagnostic, ``"none"`` when it launched nothing; on the ``split`` fallback ``last_route()`` names the per-point form that finished)."""
    return load().atx_last_gather_route().decode()


def combine_stack(op: int, inputs, outputs, *, n_pts, n_lev, pitch, layout, level_param=None, flags: int = 0) -> None:
    """Multi-input per-point operator over same-shape stacks (``atx_combine_stack``).  ``level_param``: a float64 value per level, except
    for ``COMB_LOOKUP`` where it is the table (its length, then its values); the second input of ``COMB_ORAS6`` is one field, not a stack."""
    dtype = inputs[0].dtype
    assert all(t.dtype == dtype for t in list(inputs) + list(outputs))
    ins = (c_void_p * len(inputs))(*[_ptr(t) for t in inputs])
    outs = (c_void_p * len(outputs))(*[_ptr(t) for t in outputs])
    if op == COMB_ORAS6:
        assert inputs[1].is_contiguous() and inputs[1].numel() >= n_pts
    if level_param is not None:
        assert level_param.dtype == torch.float64 and level_param.is_contiguous()
        assert level_param.numel() >= (2 if op == COMB_LOOKUP else n_lev)
    _call("atx_combine_stack", op, ins, len(inputs), outs, len(outputs), n_pts, n_lev, pitch, dtype_code(dtype), layout,
          _ptr(level_param), flags, _stream())


def pressure_at_height_stack(t, q, sp, A, B, out, *, n_pts, n_lev, pitch, layout, height: float) -> None:
    """``out[p]``: the pressure at ``height`` metres above the ground of every point, from the model-level stacks ``t`` and ``q`` (level 0
    the top one, same pitch and layout), the surface pressure ``sp`` and the half-level coefficients ``A``, ``B`` (float64, n_lev + 1
    each) — ``atx_pressure_at_height_stack``.  ``sp`` and ``out`` are contiguous ``[n_pts]`` tensors of the stacks' dtype."""
    dtype = t.dtype
    assert q.dtype == dtype and sp.dtype == dtype and out.dtype == dtype
    assert q.stride(0) == t.stride(0) == pitch
    assert sp.is_contiguous() and out.is_contiguous() and sp.numel() >= n_pts and out.numel() >= n_pts
    for c in (A, B):
        assert c.dtype == torch.float64 and c.is_contiguous() and c.numel() == n_lev + 1 and c.device == t.device
    _call("atx_pressure_at_height_stack", _ptr(t), _ptr(q), _ptr(sp), _ptr(A), _ptr(B), n_pts, n_lev, pitch, dtype_code(dtype), layout,
          float(height), _ptr(out), _stream())


def rotate_vectors_stack(x, y, x_out, y_out, frame, frame_kind: int, *, n_pts, n_lev, pitch, layout) -> None:
    """``(x_out, y_out)``: the vectors ``(x, y)`` of two stacks (same dtype, pitch and layout) mapped by the per-point table
    ``frame`` (``[n_pts, 2]`` for ``FRAME_ROTATION``, ``[n_pts, 4]`` for ``FRAME_GENERAL``, contiguous, the stacks' dtype) —
    ``atx_rotate_vectors_stack``.  ``x_out is x`` and ``y_out is y`` (in place) are allowed."""
    dtype = x.dtype
    width = 2 if frame_kind == FRAME_ROTATION else 4
    for t in (y, x_out, y_out):
        assert t.dtype == dtype and t.stride(0) == x.stride(0) == pitch
    assert frame.dtype == dtype and frame.is_contiguous() and frame.numel() == n_pts * width and frame.device == x.device
    _call("atx_rotate_vectors_stack", _ptr(x), _ptr(y), _ptr(x_out), _ptr(y_out), _ptr(frame), int(frame_kind), n_pts, n_lev, pitch,
          dtype_code(dtype), layout, _stream())


def obs_best_per_cell(date_ns, cell, values, target_ns, best, winner, *, n_cells: int, before_ns: int, after_ns: int,
                      closed_before: bool, closed_after: bool, freq_ns: int, weight: float) -> None:
    """``winner[t, c]``: the row of the observation table that target ``t`` shows in cell ``c`` (-1: none) — ``atx_obs_best_per_cell``.
    ``date_ns`` / ``cell``: int64 ``[n_obs]``; ``values``: float64 ``[n_cols, n_obs]`` (rows may be pitched); ``target_ns``: int64
    ``[n_time]``; ``best`` (scratch, int64) and ``winner`` (int32): contiguous ``[n_time, n_cells]``."""
    n_cols, n_obs = values.shape
    n_time = target_ns.numel()
    assert date_ns.dtype == cell.dtype == target_ns.dtype == best.dtype == torch.int64 and winner.dtype == torch.int32
    assert values.dtype == torch.float64 and (values.stride(1) == 1 or n_obs <= 1)
    assert date_ns.is_contiguous() and cell.is_contiguous() and target_ns.is_contiguous() and date_ns.numel() == cell.numel() == n_obs
    assert best.is_contiguous() and winner.is_contiguous() and best.numel() == winner.numel() == n_time * n_cells
    val_pitch = values.stride(0) if n_cols > 1 else max(n_obs, 1)
    _call("atx_obs_best_per_cell", _ptr(date_ns), _ptr(cell), _ptr(values), n_obs, n_cols, val_pitch, _ptr(target_ns), n_time, n_cells,
          int(before_ns), int(after_ns), int(bool(closed_before)), int(bool(closed_after)), int(freq_ns), float(weight), _ptr(best),
          _ptr(winner), _stream())


def obs_fill_stack(winner, values, out, *, n_time: int, n_cells: int, pitch: int, layout: int) -> None:
    """``out`` (float64 stack of ``n_time * n_cols`` levels over ``n_cells`` points): level ``t * n_cols + j`` =
    ``values[j, winner[t, :]]``, NaN where the winner is -1 — ``atx_obs_fill_stack``."""
    n_cols, n_obs = values.shape
    assert winner.dtype == torch.int32 and winner.is_contiguous() and winner.numel() == n_time * n_cells
    assert values.dtype == out.dtype == torch.float64 and (values.stride(1) == 1 or n_obs <= 1)
    assert out.numel() == 0 or out.stride(0) == pitch
    val_pitch = values.stride(0) if n_cols > 1 else max(n_obs, 1)
    _call("atx_obs_fill_stack", _ptr(winner), _ptr(values), n_obs, n_cols, val_pitch, n_time, n_cells, _ptr(out), pitch, layout, _stream())


def _group_order_args(order, offsets) -> tuple[int, int]:
    assert order.dtype == torch.int32 and order.is_contiguous() and offsets.dtype == torch.int64 and offsets.is_contiguous()
    assert offsets.numel() >= 1
    return order.numel(), offsets.numel() - 1


def obs_group_mean(values, order, offsets, mean, count) -> None:
    """``mean[c, g]`` / ``count[c, g]``: pandas' group mean (one Kahan sum in row order, NaN skipped) of column ``c`` of ``values``
    (float64 ``[n_cols, n_obs]``, rows may be pitched) over the rows ``order[offsets[g]:offsets[g + 1]]`` — ``atx_obs_group_mean``.
    ``order``: int32 row indices in group order (a stable sort by group); ``offsets``: int64 ``[n_groups + 1]``; ``mean`` float64 and
    ``count`` int64: ``[n_cols, n_groups]``, rows may be pitched (``out_pitch`` is ``mean.stride(0)``, the same for ``count``)."""
    n_cols, n_obs = values.shape
    n_sel, n_groups = _group_order_args(order, offsets)
    assert values.dtype == mean.dtype == torch.float64 and count.dtype == torch.int64 and (values.stride(1) == 1 or n_obs <= 1)
    assert tuple(mean.shape) == tuple(count.shape) == (n_cols, n_groups)
    assert n_groups <= 1 or (mean.stride(1) == 1 and count.stride(1) == 1)
    val_pitch = values.stride(0) if n_cols > 1 else max(n_obs, 1)
    out_pitch = max(n_groups, 1)
    if n_cols > 1:
        out_pitch = mean.stride(0)
        assert count.stride(0) == out_pitch, f"mean rows are {out_pitch} elements apart, count rows {count.stride(0)}"
    _call("atx_obs_group_mean", _ptr(values), n_obs, n_cols, val_pitch, _ptr(order), n_sel, _ptr(offsets), n_groups, _ptr(mean), _ptr(count),
          out_pitch, _stream())


def obs_group_argmin(distance, order, offsets, nearest) -> None:
    """``nearest[g]`` (int32): the first row of smallest ``distance`` (float64 ``[n_obs]``) among ``order[offsets[g]:offsets[g + 1]]`` —
    ``atx_obs_group_argmin``."""
    n_sel, n_groups = _group_order_args(order, offsets)
    assert distance.dtype == torch.float64 and distance.is_contiguous() and nearest.dtype == torch.int32 and nearest.is_contiguous()
    assert nearest.numel() == n_groups
    _call("atx_obs_group_argmin", _ptr(distance), distance.numel(), _ptr(order), n_sel, _ptr(offsets), n_groups, _ptr(nearest), _stream())


# the nine columns of atx_obs_forcings in the order of their mask bits (R: filters/tabular/add_forcings.py:51-61)
FORCINGS = ("cos_julian_day", "sin_julian_day", "cos_sza", "sin_local_time", "cos_local_time", "cos_latitude", "sin_latitude",
            "cos_longitude", "sin_longitude")
VIEW_AZIMUTH, VIEW_ZENITH = 1, 2


def _rows(*columns, n: int) -> None:
    for c in columns:
        assert c is None or (c.dtype == torch.float64 and c.is_contiguous() and c.numel() == n)


def obs_forcings(date_ns, latitude, longitude, mask: int, out) -> None:
    """``out`` (float64 ``[popcount(mask), n]``, rows may be pitched): the forcings whose bits ``mask`` holds (``FORCINGS`` order) of
    the rows ``date_ns`` (int64 nanoseconds, NaT = INT64_MIN), ``latitude``, ``longitude`` (float64 degrees) — ``atx_obs_forcings``.
    A column the mask does not need may be ``None``."""
    n = out.shape[1]
    _rows(latitude, longitude, n=n)
    assert date_ns is None or (date_ns.dtype == torch.int64 and date_ns.is_contiguous() and date_ns.numel() == n)
    assert out.dtype == torch.float64 and out.shape[0] == bin(int(mask)).count("1") and (out.stride(1) == 1 or n <= 1)
    pitch = out.stride(0) if out.shape[0] > 1 else max(n, 1)
    _call("atx_obs_forcings", _ptr(date_ns), _ptr(latitude), _ptr(longitude), n, int(mask), _ptr(out), pitch, _stream())


def obs_view_angles(latitude, longitude, sat_latitude, sat_longitude, flags: int, out) -> None:
    """``out`` (float64 ``[popcount(flags), n]``): the viewing azimuth (``VIEW_AZIMUTH``) and / or zenith (``VIEW_ZENITH``) in degrees,
    azimuth first — ``atx_obs_view_angles``.  All four inputs float64 ``[n]`` in degrees."""
    n = out.shape[1]
    _rows(latitude, longitude, sat_latitude, sat_longitude, n=n)
    assert out.dtype == torch.float64 and out.shape[0] == bin(int(flags)).count("1") and (out.stride(1) == 1 or n <= 1)
    pitch = out.stride(0) if out.shape[0] > 1 else max(n, 1)
    _call("atx_obs_view_angles", _ptr(latitude), _ptr(longitude), _ptr(sat_latitude), _ptr(sat_longitude), n, int(flags), _ptr(out), pitch,
          _stream())


def obs_planck_bt(radiance, a, b, out) -> None:
    """``out[c, i] = b[c] / log1p(a[c] / max(radiance[c, i] * 1e-2, 1e-300))`` for float64 ``[n_ch, n]`` radiances (rows may be
    pitched) and the per-channel tables ``a``, ``b`` (float64 ``[n_ch]``) — ``atx_obs_planck_bt``.  ``out is radiance`` is allowed."""
    n_ch, n = radiance.shape
    assert radiance.dtype == out.dtype == a.dtype == b.dtype == torch.float64 and tuple(out.shape) == (n_ch, n)
    assert a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel() == n_ch
    assert (radiance.stride(1) == 1 and out.stride(1) == 1) or n <= 1
    in_pitch = radiance.stride(0) if n_ch > 1 else max(n, 1)
    out_pitch = out.stride(0) if n_ch > 1 else max(n, 1)
    _call("atx_obs_planck_bt", _ptr(radiance), n, n_ch, in_pitch, _ptr(a), _ptr(b), _ptr(out), out_pitch, _stream())


HEALPIX_RING, HEALPIX_NEST = 0, 1  # atx_healpix_scheme


def healpix_ang2pix(longitude, latitude, nside: int, nest: bool, out, n_bad) -> None:
    """``out[i]`` (int64 ``[n]``): the HEALPix pixel of ``(longitude[i], latitude[i])`` (float64 ``[n]``, degrees) at ``nside``, NESTED
    or RING — ``atx_healpix_ang2pix``.  A row without a pixel (NaN or out-of-range latitude, non-finite longitude) holds -1;
    ``n_bad`` (int64 ``[1]`` on the device) counts them.  Does not synchronise."""
    n = out.numel()
    _rows(longitude, latitude, n=n)
    assert out.dtype == torch.int64 and out.is_contiguous() and n_bad.dtype == torch.int64 and n_bad.numel() == 1
    _call("atx_healpix_ang2pix", _ptr(longitude), _ptr(latitude), n, int(nside), HEALPIX_NEST if nest else HEALPIX_RING, _ptr(out), _ptr(n_bad),
          _stream())


FILL_TIE_LATITUDE, FILL_TIE_LONGITUDE = 1, 2  # the bits of atx_obs_fill_heights' flags


def obs_fill_heights(latitude, longitude, altitude, lat_axis, lat_perm, lon_axis, lon_perm, heights, out, flags, counters) -> None:
    """``out[r]`` (float64 ``[n]``): ``altitude[r]`` bit for bit, or — where it is NaN or 9999.0 — ``heights[i, j]`` at the axis entries
    nearest to ``(latitude[r], longitude[r])`` by cKDTree's measure — ``atx_obs_fill_heights``.  The axes (float64) come sorted ascending
    with their int32 permutations back to file order; ``heights``: float32 or float64 ``[n_lat, n_lon]`` in file order (rows may be
    pitched).  ``flags`` (uint8 ``[n]``): ``FILL_TIE_*`` bits where an axis has two equally near entries and the caller has to answer;
    ``counters`` (int64 ``[3]`` on the device, set by the call): rows given a value, flagged rows, rows to fill whose coordinates are not
    finite.  Does not synchronise."""
    n = out.numel()
    _rows(latitude, longitude, altitude, out, n=n)
    n_lat, n_lon = lat_axis.numel(), lon_axis.numel()
    for axis, perm in ((lat_axis, lat_perm), (lon_axis, lon_perm)):
        assert axis.dtype == torch.float64 and perm.dtype == torch.int32 and axis.is_contiguous() and perm.is_contiguous()
        assert axis.dim() == 1 and perm.numel() == axis.numel()
    assert heights.dim() == 2 and tuple(heights.shape) == (n_lat, n_lon) and (heights.stride(1) == 1 or n_lon <= 1)
    assert flags.dtype == torch.uint8 and flags.is_contiguous() and flags.numel() == n
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() == 3
    pitch = heights.stride(0) if n_lat > 1 else max(n_lon, 1)
    _call("atx_obs_fill_heights", _ptr(latitude), _ptr(longitude), _ptr(altitude), n, _ptr(lat_axis), _ptr(lat_perm), n_lat, _ptr(lon_axis),
          _ptr(lon_perm), n_lon, _ptr(heights), pitch, dtype_code(heights.dtype), _ptr(out), _ptr(flags), _ptr(counters), _stream())


MAX_COLUMN_OPS = 16
# the ATX_COLOP_* codes by the reference's function names (R: filters/tabular/apply_column_transformations.py:31-42, in its order)
COLUMN_OPS = {"log": 0, "log1p": 1, "safe_log": 2, "sqrt": 3, "exp": 4, "abs": 5, "sin": 6, "sin_deg": 7, "cos": 8, "cos_deg": 9}
# the second family of ATX_COLOP_* codes: the row operations of the tabular QC filters (include/atx.h; csrc/atx_obs_row_program.hip).  A
# program is all COLUMN_OPS or all ROW_OPS.  The binary ones (cmp_gt and above) take the result of the operation before them as y.
ROW_OPS = {"scalar": 16, "copy": 17, "is_nan": 18, "not": 19, "cmp_gt": 20, "cmp_lt": 21, "cmp_eq": 22, "cmp_ne": 23, "cmp_ge": 24,
           "cmp_le": 25, "abs_gt": 26, "and": 27, "or": 28, "nan_where": 29, "clip_low": 30, "clip_high": 31, "fill_nan": 32}


def obs_column_ops(ops, n: int) -> None:
    """One launch of ``atx_obs_column_ops`` over ``n`` rows.  ``ops``: 1 .. ``MAX_COLUMN_OPS`` tuples ``(code, src, column, out)`` —
    ``code`` an ATX_COLOP_* value; ``src`` -1 to read ``column`` (a float64 device row of ``n``), or the index of the earlier
    operation whose result is taken (``column`` is then ignored and may be ``None``); ``out`` a float64 device row of ``n`` or ``None``
    for an intermediate.  ``out`` may be ``column``.  The ``column`` of a ``ROW_OPS["scalar"]`` operation is a float64 device tensor of
    which element 0 alone is read.  Does not synchronise."""
    for code, src, column, out in ops:
        if int(code) == ROW_OPS["scalar"] and column is not None:
            assert column.dtype == torch.float64 and column.is_contiguous() and column.numel() >= 1, "a scalar is a float64 device tensor of one element"
            _rows(None, out, n=n)
            continue
        _rows(column if src < 0 else None, out, n=n)
    k = len(ops)
    codes = (c_int32 * k)(*[int(o[0]) for o in ops])
    srcs = (c_int32 * k)(*[int(o[1]) for o in ops])
    ins = (c_void_p * k)(*[_ptr(o[2]) if o[1] < 0 else None for o in ops])
    outs = (c_void_p * k)(*[_ptr(o[3]) for o in ops])
    _call("atx_obs_column_ops", k, codes, srcs, ins, outs, n, _stream())


# the atx_expr_op codes (include/atx.h; csrc/atx_obs_row_expr.hip) and the limits of one row-expression program
EXPR_OPS = {"push_col": 0, "push_const": 1, "add": 2, "sub": 3, "mul": 4, "div": 5, "neg": 6, "abs": 7, "round_f32": 8, "cmp_gt": 9,
            "cmp_lt": 10, "cmp_eq": 11, "cmp_ne": 12, "cmp_ge": 13, "cmp_le": 14, "in_set": 15, "and": 16, "or": 17, "not": 18, "dup": 19,
            "swap": 20, "nan_where": 21}
EXPR_MAX_INPUTS, EXPR_MAX_INSTR, EXPR_MAX_CONSTS, EXPR_MAX_STACK, EXPR_MAX_RESULTS, EXPR_CHUNK_ROWS = 16, 32, 64, 8, 4, 256


def obs_row_expr(instructions, inputs, consts, outs, n: int, keep_words=None, chunk_counts=None) -> None:
    """One launch of ``atx_obs_row_expr`` over ``n`` rows.
    ``instructions``: tuples ``(code, arg0, arg1)`` in postfix order, ``code`` an ``EXPR_OPS`` value — ``push_col`` takes the index of an
    input, ``push_const`` of a constant, ``in_set`` the start and the count of a slice of the constants, ``dup`` the distance below the
    top; ``inputs``: float64 device rows of ``n``; ``consts``: floats; ``outs``: up to ``EXPR_MAX_RESULTS`` float64 device rows of ``n``,
    which take the stack slots 0 .. from the bottom (an ``out`` may be an input).  With ``keep_words`` (int64 ``[ceil(n / 64)]``) and
    ``chunk_counts`` (int64 ``[ceil(n / EXPR_CHUNK_ROWS)]``) the slot on top of the value results is the keep condition: one bit per
    row, one count per chunk.  The limits (``EXPR_MAX_*``), the indices and the stack are checked by the library: ``ValueError``.  Does
    not synchronise."""
    for t in (*inputs, *outs):
        _rows(t, None, n=n)
    if (keep_words is None) != (chunk_counts is None):
        raise ValueError("obs_row_expr: keep_words and chunk_counts go together")
    if keep_words is not None:
        assert keep_words.dtype == torch.int64 and keep_words.is_contiguous() and keep_words.numel() == (n + 63) // 64
        assert chunk_counts.dtype == torch.int64 and chunk_counts.is_contiguous()
        assert chunk_counts.numel() == (n + EXPR_CHUNK_ROWS - 1) // EXPR_CHUNK_ROWS
    k = len(instructions)
    code, arg0, arg1 = ((c_int32 * max(k, 1))(*[int(i[field]) for i in instructions]) for field in range(3))
    _call("atx_obs_row_expr", k, code, arg0, arg1, len(inputs), (c_void_p * max(len(inputs), 1))(*[_ptr(t) for t in inputs]), len(consts),
          (c_double * max(len(consts), 1))(*[float(c) for c in consts]), len(outs), (c_void_p * max(len(outs), 1))(*[_ptr(t) for t in outs]),
          int(keep_words is not None), _ptr(keep_words), _ptr(chunk_counts), n, _stream())


def obs_keep_positions(keep_words, chunk_offsets, n: int, positions) -> None:
    """``positions`` (int64 ``[count]``): the rows whose bit is set in ``keep_words``, ascending (``atx_obs_keep_positions``).
    ``chunk_offsets``: the exclusive prefix sum of ``obs_row_expr``'s ``chunk_counts``.  Does not synchronise."""
    for t in (keep_words, chunk_offsets, positions):
        assert t.dtype == torch.int64 and t.is_contiguous()
    assert keep_words.numel() == (n + 63) // 64 and chunk_offsets.numel() == (n + EXPR_CHUNK_ROWS - 1) // EXPR_CHUNK_ROWS
    _call("atx_obs_keep_positions", _ptr(keep_words), _ptr(chunk_offsets), n, _ptr(positions), positions.numel(), _stream())


MAX_ROWSET_COLUMNS = 16
# atx_key_dtype by torch dtype; KEY_DATETIME is int64 nanoseconds with NaT = INT64_MIN and has to be asked for
KEY_F64, KEY_F32, KEY_I64, KEY_I32, KEY_I16, KEY_I8, KEY_U8, KEY_BOOL, KEY_DATETIME = range(9)
KEY_DTYPES = {torch.float64: KEY_F64, torch.float32: KEY_F32, torch.int64: KEY_I64, torch.int32: KEY_I32, torch.int16: KEY_I16,
              torch.int8: KEY_I8, torch.uint8: KEY_U8, torch.bool: KEY_BOOL}


def obs_order_key(column, key, code: int | None = None) -> None:
    """``key[i]`` (int64 ``[n]``): the order key of ``column[i]`` by pandas' rule — ``-0.0`` and ``0.0`` one key, every NaN / NaT one
    key and the last, integers as integers — ``atx_obs_order_key``.  ``code``: a ``KEY_*`` value, by default the one of the column's
    dtype (``KEY_DTYPES``); ``KEY_DATETIME`` for int64 nanoseconds.  Does not synchronise."""
    if code is None:
        if column.dtype not in KEY_DTYPES:
            raise ValueError(f"no order key for a {column.dtype} column (float64, float32, int64, int32, int16, int8, uint8, bool)")
        code = KEY_DTYPES[column.dtype]
    n = key.numel()
    assert column.is_contiguous() and column.numel() == n and key.dtype == torch.int64 and key.is_contiguous()
    assert code != KEY_DATETIME or column.dtype == torch.int64
    _call("atx_obs_order_key", _ptr(column), n, int(code), _ptr(key), _stream())


def obs_mark_first(keys, order, keep, accumulate: bool = False) -> None:
    """``keep[order[i]] = (i == 0) or any(key[order[i]] != key[order[i - 1]] for key in keys)`` for 1 .. ``MAX_ROWSET_COLUMNS`` int64
    key rows — ``atx_obs_mark_first``.  ``order``: int64 ``[n]``, a permutation; ``keep``: uint8 ``[n]``, written (``accumulate``: only
    ever set).  Does not synchronise."""
    n = keep.numel()
    for t in (*keys, order):
        assert t.dtype == torch.int64 and t.is_contiguous() and t.numel() == n
    assert keep.dtype == torch.uint8 and keep.is_contiguous()
    k = len(keys)
    table = (c_void_p * max(k, 1))(*[_ptr(t) for t in keys])
    _call("atx_obs_mark_first", k, table, _ptr(order), n, 1 if accumulate else 0, _ptr(keep), _stream())


def obs_take_rows(columns, outs, rows, n_bad) -> None:
    """``outs[c][i] = columns[c][rows[i]]`` for 1 .. ``MAX_ROWSET_COLUMNS`` device rows of 1, 2, 4 or 8 bytes per element, any mix —
    ``atx_obs_take_rows``.  ``rows``: int64 ``[n_out]``; a row index outside the table writes nothing and is counted in ``n_bad`` (int64
    ``[1]`` on the device, set by the call when ``n_out > 0``).  Does not synchronise."""
    n_out = rows.numel()
    n_in = columns[0].numel() if columns else 0
    assert rows.dtype == torch.int64 and rows.is_contiguous() and n_bad.dtype == torch.int64 and n_bad.numel() == 1
    for c, o in zip(columns, outs):
        assert c.is_contiguous() and o.is_contiguous() and c.numel() == n_in and o.numel() == n_out and c.dtype == o.dtype
    k = len(columns)
    assert len(outs) == k
    ins = (c_void_p * max(k, 1))(*[_ptr(c) for c in columns])
    dst = (c_void_p * max(k, 1))(*[_ptr(o) for o in outs])
    width = (c_int32 * max(k, 1))(*[c.element_size() for c in columns])
    _call("atx_obs_take_rows", k, ins, dst, width, _ptr(rows), n_out, n_in, _ptr(n_bad), _stream())


def mask_build(m, mask, *, n, stride=1, cmp, threshold=0.0) -> None:
    assert mask.dtype == torch.uint8
    _call("atx_mask_build", _ptr(m), stride, _ptr(mask), n, cmp, float(threshold), dtype_code(m.dtype), _stream())


def mask_count(mask, n: int | None = None) -> int:
    n = mask.numel() if n is None else n
    count = torch.zeros(1, dtype=torch.int64, device=mask.device)
    _call("atx_mask_count", _ptr(mask), n, _ptr(count), _stream())
    return int(count.item())


def mask_to_index(mask, n: int | None = None) -> torch.Tensor:
    """Ascending int32 positions of the set mask bytes (stable compaction; synchronises)."""
    n = mask.numel() if n is None else n
    slot = _Scratch.of(mask.device)
    workspace = slot.room(max(load().atx_mask_to_index_workspace(n), 16))
    index = torch.empty(max(n, 1), dtype=torch.int32, device=mask.device)  # the caller keeps (a view of) this one
    # the count lands in the pinned host cell straight from the scan kernel
    _call("atx_mask_to_index", _ptr(mask), n, _ptr(index), slot.host_count.data_ptr(), _ptr(workspace), workspace.numel(), _stream())
    slot.wait()
    return index[: int(slot.host_count[0])]


class KnnIndex:
    """A device k-NN index over source points (``atx_knn_build`` / ``atx_knn_query``).  ``workspace``: the caller's uint8 buffer
    (256-byte aligned, at least ``atx_knn_workspace_bytes(n_src)`` bytes, of which exactly that many are used) instead of one of
    the index's own."""

    def __init__(self, src_xyz: torch.Tensor, workspace: torch.Tensor | None = None) -> None:
        assert src_xyz.dtype == torch.float64 and src_xyz.dim() == 2 and src_xyz.shape[1] == 3 and src_xyz.is_contiguous()
        self.n_src = src_xyz.shape[0]
        nbytes = load().atx_knn_workspace_bytes(self.n_src)
        if nbytes == 0:
            raise ValueError(f"cannot index {self.n_src} source points")
        if workspace is None:
            self.workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=src_xyz.device)
            shift = (-self.workspace.data_ptr()) % 256
        else:
            assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == src_xyz.device
            assert workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0
            self.workspace, shift = workspace, 0
        self._ws = self.workspace[shift: shift + nbytes]
        _call("atx_knn_build", _ptr(src_xyz), self.n_src, _ptr(self._ws), nbytes, _stream())

    def query(self, tgt_xyz: torch.Tensor, k: int, out: tuple[torch.Tensor, torch.Tensor] | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """``(indices int32 [n, k], squared distances float64 [n, k])``, nearest first; into ``out`` when given."""
        assert tgt_xyz.dtype == torch.float64 and tgt_xyz.dim() == 2 and tgt_xyz.shape[1] == 3 and tgt_xyz.is_contiguous()
        n = tgt_xyz.shape[0]
        if out is None:
            idx = torch.empty((n, k), dtype=torch.int32, device=tgt_xyz.device)
            d2 = torch.empty((n, k), dtype=torch.float64, device=tgt_xyz.device)
        else:
            idx, d2 = out
            assert idx.dtype == torch.int32 and d2.dtype == torch.float64 and tuple(idx.shape) == tuple(d2.shape) == (n, k)
            assert idx.is_contiguous() and d2.is_contiguous() and idx.device == d2.device == tgt_xyz.device
        _call("atx_knn_query", _ptr(self._ws), self.n_src, _ptr(tgt_xyz), n, k, _ptr(idx), _ptr(d2), _stream())
        return idx, d2


def cutout_inside(global_xyz: torch.Tensor, lam_xyz: torch.Tensor, neighbours: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 [n]: the ray through each global point hits a triangle of its nearest LAM points (``atx_cutout_inside``); into ``out``
    (uint8 ``[n]``) when given."""
    assert global_xyz.dtype == lam_xyz.dtype == torch.float64 and neighbours.dtype == torch.int32
    n, k = neighbours.shape
    if out is None:
        inside = torch.empty(max(n, 1), dtype=torch.uint8, device=global_xyz.device)
    else:
        assert out.dtype == torch.uint8 and out.numel() == n and out.is_contiguous() and out.device == global_xyz.device
        inside = out
    _call("atx_cutout_inside", _ptr(global_xyz), n, _ptr(lam_xyz), lam_xyz.shape[0], _ptr(neighbours), k, _ptr(inside), _stream())
    return inside[:n]


class _Scratch:
    """Per-(device, stream) slots for the small synchronous calls (``reduce``, ``reduce_stack``, ``mask_to_index``): pinned HOST
    cells the kernels write their result into directly (pinned memory is device-visible at the same address), the zeroed
    workspace of the ticketed reduction, the event the host waits on and a growing scratch buffer.  Such a call is then its
    launch(es) and ONE event wait — no allocation, no fill, no initialisation launch, no copy back, no blocking ``.item()``
    (``reduce`` of one 26 MB field: 45 us -> see tools/small_case_bench.py).  Slots are per (device, stream, host thread)."""

    _slots: dict = {}

    def __init__(self, device) -> None:
        self.result = torch.zeros(2, dtype=torch.float64, device=device)
        self.host = torch.zeros(2, dtype=torch.float64).pin_memory()
        self.host_count = torch.zeros(1, dtype=torch.int64).pin_memory()
        self.reduce_ws = torch.empty(load().atx_reduce_workspace() // 8 + 1, dtype=torch.int64, device=device)
        self.event = torch.cuda.Event()
        self.workspace = torch.empty(4096, dtype=torch.uint8, device=device)

    @classmethod
    def of(cls, device) -> "_Scratch":
        # per host thread as well: a producer thread (prefetch) and the consumer may enqueue on the same stream
        key = (device.index if device.index is not None else torch.cuda.current_device(), _stream(), threading.get_ident())
        slot = cls._slots.get(key)
        if slot is None:
            if len(cls._slots) >= 64:  # streams come and go
                cls._slots.clear()
            slot = cls._slots[key] = cls(device)
        return slot

    def wait(self) -> None:
        self.event.record()
        self.event.synchronize()

    def room(self, n_bytes: int) -> torch.Tensor:
        if self.workspace.numel() < n_bytes:
            self.workspace = torch.empty(max(n_bytes, 2 * self.workspace.numel()), dtype=torch.uint8, device=self.workspace.device)
        return self.workspace


# ATX_REDUCE_WORKSPACE=0 takes the library's route without a workspace (per-workgroup atomics on a device cell + a copy back).
_REDUCE_TICKET = os.environ.get("ATX_REDUCE_WORKSPACE", "1") == "1"


def _reduce_ws(slot: "_Scratch"):
    if _REDUCE_TICKET:
        return _ptr(slot.reduce_ws), slot.reduce_ws.numel() * 8, slot.host.data_ptr()
    return None, 0, _ptr(slot.result)


def _reduction_result(slot: _Scratch, red: int):
    if not _REDUCE_TICKET:
        slot.host.copy_(slot.result, non_blocking=True)
    slot.wait()
    if red == RED_MINMAX:
        return float(slot.host[0]), float(slot.host[1])  # both from one pass, one wait
    return float(slot.host[0])


def reduce(x, red: int, n: int | None = None):
    """``atx_reduce``; ``RED_MINMAX`` returns ``(minimum, maximum)`` from one pass."""
    n = x.numel() if n is None else n
    slot = _Scratch.of(x.device)
    ws, ws_bytes, result = _reduce_ws(slot)
    _call("atx_reduce", _ptr(x), n, red, result, dtype_code(x.dtype), ws, ws_bytes, _stream())
    return _reduction_result(slot, red)


def reduce_stack(x, red: int, *, n_pts: int, n_lev: int, pitch: int, layout: int):
    """``atx_reduce`` over the elements of a pitched stack (padding excluded); ``RED_MINMAX``: ``(minimum, maximum)``."""
    slot = _Scratch.of(x.device)
    ws, ws_bytes, result = _reduce_ws(slot)
    _call("atx_reduce_stack", _ptr(x), n_pts, n_lev, pitch, red, result, dtype_code(x.dtype), layout, ws, ws_bytes, _stream())
    return _reduction_result(slot, red)


def select_levels(src, dst, level_map, *, n_pts, n_src_lev, src_pitch, dst_pitch, layout) -> None:
    """dst level j = src level ``level_map[j]`` (negative: leave dst level j alone); ``level_map`` is a host sequence."""
    assert src.dtype == dst.dtype
    lm = (ctypes.c_int32 * len(level_map))(*[int(l) for l in level_map])
    _call("atx_select_levels", _ptr(src), _ptr(dst), ctypes.cast(lm, c_void_p), len(level_map), n_pts, n_src_lev,
          src_pitch, dst_pitch, dtype_code(src.dtype), layout, _stream())


def stream_copy(src, dst) -> None:
    """``atx_stream_copy``: the library's fixed reference streaming copy (calibration / ceiling measurements)."""
    n_bytes = src.numel() * src.element_size()
    assert dst.numel() * dst.element_size() == n_bytes and src.is_contiguous() and dst.is_contiguous()
    _call("atx_stream_copy", _ptr(src), _ptr(dst), n_bytes, _stream())


class Comm:
    """An RCCL communicator through the C ABI (``atx_comm_*``): one per process, bound to the current device.

    ``Comm.unique_id()`` on rank 0, the 128 bytes handed to every rank out of band, then ``Comm(world, rank, id)``
    everywhere (collective).  Calls enqueue on torch's current stream."""

    def __init__(self, world: int, rank: int, unique_id: bytes) -> None:
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError(f"an RCCL unique id has {COMM_ID_BYTES} bytes, got {len(unique_id)}")
        handle = c_void_p()
        buf = ctypes.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        _call("atx_comm_init", ctypes.byref(handle), int(world), int(rank), ctypes.cast(buf, c_void_p))
        self._handle = handle
        self.world, self.rank = int(world), int(rank)

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        _call("atx_comm_unique_id", ctypes.cast(buf, c_void_p))
        return buf.raw

    @staticmethod
    def rccl_version() -> int:
        v = load().atx_comm_version()
        if v < 0:
            LIBRARY.check("atx_comm_version", v)
        return v

    def bcast(self, t: torch.Tensor, root: int) -> None:
        """``t`` (contiguous, in HBM) of rank ``root`` onto every rank, in place."""
        assert t.is_contiguous()
        _call("atx_bcast", self._handle, _ptr(t), t.numel() * t.element_size(), int(root), _stream())

    def all_gather(self, mine: torch.Tensor, everyone: torch.Tensor) -> None:
        """``mine`` (contiguous) of every rank into ``everyone`` (``world`` times its size): slot ``p`` holds rank ``p``'s."""
        assert mine.is_contiguous() and everyone.is_contiguous()
        n_bytes = mine.numel() * mine.element_size()
        assert everyone.numel() * everyone.element_size() == self.world * n_bytes
        _call("atx_all_gather", self._handle, _ptr(mine), _ptr(everyone), n_bytes, _stream())

    def exchange(self, send: list, recv: list) -> None:
        """``send[p]`` goes to rank ``p``, ``recv[p]`` is filled by rank ``p``; ``None`` / empty tensors skip the pair."""
        assert len(send) == len(recv) == self.world

        def table(tensors):
            ptrs = (c_void_p * self.world)()
            sizes = (c_int64 * self.world)()
            for p, t in enumerate(tensors):
                if t is not None and t.numel():
                    assert t.is_contiguous()
                    ptrs[p], sizes[p] = _ptr(t), t.numel() * t.element_size()
            return ptrs, sizes

        sp, sb = table(send)
        rp, rb = table(recv)
        _call("atx_exchange", self._handle, sp, sb, rp, rb, _stream())

    def gather_shards(self, full: torch.Tensor, byte_offsets: list[int]) -> None:
        """Every rank has filled its byte range ``[byte_offsets[rank], byte_offsets[rank + 1])`` of ``full``; afterwards all have all."""
        assert full.is_contiguous() and len(byte_offsets) == self.world + 1
        assert byte_offsets[-1] <= full.numel() * full.element_size()
        offs = (c_int64 * (self.world + 1))(*[int(o) for o in byte_offsets])
        _call("atx_gather_shards", self._handle, _ptr(full), offs, _stream())

    def destroy(self) -> None:
        if self._handle is not None:
            handle, self._handle = self._handle, None
            _call("atx_comm_destroy", handle)

    def __del__(self) -> None:  # best effort; explicit destroy() is the documented way
        try:
            self.destroy()
        except Exception:
            pass


def relayout(src, dst, *, n_pts, n_lev, src_pitch, dst_pitch, src_layout, dst_layout) -> None:
    assert src.dtype == dst.dtype
    _call(
        "atx_relayout", _ptr(src), _ptr(dst), n_pts, n_lev, src_pitch, dst_pitch, src_layout, dst_layout,
        dtype_code(src.dtype), _stream(),
    )
