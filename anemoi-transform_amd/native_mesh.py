"""ctypes binding of libatx_mesh — point location in a triangulated source grid (``include/atx_mesh.h``), a library of its own next
to libatx.

There is no CPU fallback: if ``lib/libatx_mesh.so`` is missing, or a tensor handed to a wrapper does not live in HBM, the call raises.
"""

from __future__ import annotations

from ctypes import c_char_p, c_int, c_int32, c_int64, c_void_p
from typing import Any

import torch

from ._binding import EINVAL, OK, Library  # noqa: F401 - the status codes are part of this module's names

FOUND, UNDECIDED, OUTSIDE, MALFORMED = 0, 1, 2, 3  # the status codes of atx_mesh_locate
MAX_STEPS = 1 << 20  # ATX_MESH_MAX_STEPS

# every symbol include/atx_mesh.h declares: name -> (restype, argtypes)
SIGNATURES: dict[str, tuple[Any, list[Any]]] = {
    "atx_mesh_version": (c_int, []),
    "atx_mesh_last_error": (c_char_p, []),
    "atx_mesh_locate": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

LIBRARY = Library("libatx_mesh.so", "ATX_MESH_LIBRARY", SIGNATURES, "atx_mesh_last_error")
lib_path = LIBRARY.path  # ``lib/libatx_mesh.so`` next to this file; ``ATX_MESH_LIBRARY`` overrides it
load = LIBRARY.load  # libatx_mesh.so, opened once with every prototype declared; raises if it is absent or lacks a symbol of the header


def _check(name: str, t: torch.Tensor, dtype: torch.dtype, shape: tuple[int, ...], dev: torch.device) -> None:
    if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda or t.device != dev:
        raise ValueError(f"{name} must be a contiguous {dtype} {list(shape)} in HBM on {dev}, got {t.dtype} {list(t.shape)} on {t.device}")


class Mesh:
    """A triangulation in HBM (``include/atx_mesh.h``): ``src_xyz`` float64 ``[n_src, 3]``, ``tri`` / ``nbr`` int32 ``[n_tri, 3]``,
    ``flag`` uint8 ``[n_tri]``, all on the device of ``src_xyz``."""

    def __init__(self, src_xyz: torch.Tensor, tri: torch.Tensor, nbr: torch.Tensor, flag: torch.Tensor) -> None:
        if src_xyz.dim() != 2 or tri.dim() != 2 or not src_xyz.is_cuda:
            raise ValueError("a mesh is src_xyz [n_src, 3], tri [n_tri, 3], nbr [n_tri, 3] and flag [n_tri] in HBM")
        n_src, n_tri, dev = src_xyz.shape[0], tri.shape[0], src_xyz.device
        if n_src < 1 or n_tri < 1:
            raise ValueError("a mesh has at least one point and one triangle")
        _check("src_xyz", src_xyz, torch.float64, (n_src, 3), dev)
        _check("tri", tri, torch.int32, (n_tri, 3), dev)
        _check("nbr", nbr, torch.int32, (n_tri, 3), dev)
        _check("flag", flag, torch.uint8, (n_tri,), dev)
        self.src_xyz, self.tri, self.nbr, self.flag, self.n_src, self.n_tri, self.device = src_xyz, tri, nbr, flag, n_src, n_tri, dev


def locate(mesh: Mesh, tgt_xyz: torch.Tensor, seed: torch.Tensor, max_steps: int = 64):
    """``atx_mesh_locate`` on the current stream: ``(tri_out int32 [n], w float64 [n, 3], status int32 [n], steps int32 [n])`` in HBM
    for the targets ``tgt_xyz`` (float64 ``[n, 3]``) walked from the triangles ``seed`` (int32 ``[n]``)."""
    n = tgt_xyz.shape[0] if tgt_xyz.dim() == 2 else -1
    _check("tgt_xyz", tgt_xyz, torch.float64, (n, 3), mesh.device)
    _check("seed", seed, torch.int32, (n,), mesh.device)
    if not 0 <= int(max_steps) <= MAX_STEPS:
        raise ValueError(f"max_steps = {max_steps} is outside 0 .. {MAX_STEPS}")
    tri_out = torch.empty(n, dtype=torch.int32, device=mesh.device)
    w = torch.empty((n, 3), dtype=torch.float64, device=mesh.device)
    status = torch.empty(n, dtype=torch.int32, device=mesh.device)
    steps = torch.empty(n, dtype=torch.int32, device=mesh.device)
    handle = load()
    with torch.cuda.device(mesh.device):
        stream = torch.cuda.current_stream().cuda_stream
        code = handle.atx_mesh_locate(mesh.src_xyz.data_ptr(), mesh.n_src, mesh.tri.data_ptr(), mesh.nbr.data_ptr(), mesh.flag.data_ptr(),
                                      mesh.n_tri, tgt_xyz.data_ptr(), seed.data_ptr(), n, int(max_steps), tri_out.data_ptr(), w.data_ptr(),
                                      status.data_ptr(), steps.data_ptr(), stream)
    LIBRARY.check("atx_mesh_locate", code)
    return tri_out, w, status, steps
