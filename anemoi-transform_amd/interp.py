"""Index / weight precompute for the regrid filter (CPU, one-off per grid pair).

The reference builds its gather indices with ``scipy.spatial.cKDTree`` on
unit-sphere coordinates (R: spatial.py:132-167, 587-635) and reads interpolation
matrices written by ``anemoi-transform make-regrid-file`` as ``.npz`` CSR
triplets (R: commands/make-regrid-file.py:150-160, filters/fields/regrid.py:281-290).
Both stay on the CPU here (one-off, seconds); their OUTPUTS
feed the HIP gather kernels.  The external ``mir`` binary the reference shells
out to for bilinear matrices is not available offline, so this module also
generates k-NN inverse-distance and bilinear matrices in the same npz format.
"""

from __future__ import annotations

import logging
from collections import OrderedDict
from typing import Any

import numpy as np

from .grids import gaussian_latitudes, octahedral_row_lengths

__all__ = [
    "unit_sphere_xyz",
    "nearest_grid_points",
    "nearest_grid_points_device",
    "device_knn",
    "knn_inverse_distance",
    "ell_to_csr",
    "csr_uniform_k",
    "bilinear_octahedral",
    "bilinear_rows",
    "box_row_table",
    "box_average_rows",
    "triangulate_sphere",
    "locate_walk_host",
    "locate_brute_host",
    "linear_triangulated",
    "save_matrix_npz",
    "load_matrix_npz",
]


LOG = logging.getLogger(__name__)
_knn_engine: str | None = None


def knn_engine() -> str:
    """``"ckdtree"`` (default: the reference's own builder) or ``"device"`` (``atx_knn_*`` on the GPU with
    equidistant candidates settled by cKDTree — the same table; set with ``set_knn_engine`` or ``ATX_KNN=device``)."""
    import os

    return _knn_engine or os.environ.get("ATX_KNN", "ckdtree")


def set_knn_engine(name: str | None) -> None:
    global _knn_engine
    if name not in (None, "ckdtree", "device"):
        raise ValueError(f"unknown k-NN engine {name!r}")
    _knn_engine = name


def unit_sphere_xyz(latitudes: np.ndarray, longitudes: np.ndarray) -> np.ndarray:
    """``[N, 3]`` Cartesian coordinates on the unit sphere (R: spatial.py:132-167)."""
    phi = np.deg2rad(np.asarray(latitudes, dtype=np.float64))
    lda = np.deg2rad(np.asarray(longitudes, dtype=np.float64))
    cos_phi = np.cos(phi)
    return np.array((cos_phi * np.cos(lda), cos_phi * np.sin(lda), np.sin(phi))).transpose()


MAX_DEVICE_K = 16  # atx_knn_query keeps up to 17 neighbours: these 16 plus the look-ahead one of the tie detection


# ---- remembered k-NN tables ---------------------------------------------------------------------------------------------------
# `cKDTree(src).query(tgt, k)` (R: spatial.py:628-632) is a pure function of the two point sets, k and the distance bound, and it
# is the expensive part of building a `regrid(method="nearest")` filter or a k-NN matrix: 2.4 s for O1280 -> 0.25 degree on the
# MI355X box's host, of which the tree build is 1.5 s — and a job builds the same filter for every variable / date it handles.
# Tables are therefore remembered per (source hash, target hash, k, bound, tie order): in the process (LRU, bounded in bytes)
# and on disk in the MIR-matrix npz layout (R: regrid.py:281-290: matrix_data = the chord distances, matrix_indices,
# matrix_indptr, matrix_shape) under ATX_CACHE_DIR (default ~/.cache/anemoi-transform-amd; "off" disables the files); the host
# cKDTree that settles equidistant candidates for the device search is remembered per source grid as well.
_TABLES: "OrderedDict[tuple, tuple[np.ndarray, np.ndarray]]" = OrderedDict()
_TABLES_MAX_BYTES = 1 << 30
_TREES: "OrderedDict[str, Any]" = OrderedDict()
_TREES_MAX = 2
_DISK_MIN_ENTRIES = 100_000  # smaller tables are rebuilt faster than a file is found
_cache_stats = {"memory_hits": 0, "disk_hits": 0, "misses": 0, "trees_built": 0}
KNN_TABLE_FORMAT = 2  # bump when the file layout OR the device search's tie / ordering logic changes: older files are then ignored
_cache_dir_announced = False


def _library_version() -> int:
    """``ATX_VERSION`` of the loaded libatx.so, 0 when the library has not been loaded (host-only use)."""
    try:
        from . import native

        handle = native.LIBRARY.handle
        return int(handle.atx_version()) if handle is not None else 0
    except Exception:  # noqa: BLE001 - the version is a label in the file, never a reason to fail a table build
        return 0


def points_hash(*arrays: np.ndarray) -> str:
    """128-bit content hash of float64 coordinate arrays (xxh3 when the module is there: 17 ms for O1280; blake2b otherwise)."""
    try:
        import xxhash

        h = xxhash.xxh3_128()
    except ImportError:  # pragma: no cover - depends on the installation
        import hashlib

        h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=np.float64)
        h.update(str(a.shape).encode())
        h.update(a.data)
    return h.hexdigest()


def knn_cache_dir() -> str | None:
    import os

    d = os.environ.get("ATX_CACHE_DIR")
    if d is not None and d.strip().lower() in ("", "0", "off", "none", "false"):
        return None
    if d is None:
        d = os.path.join(os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache"), "anemoi-transform-amd")
    return os.path.join(d, "knn")


def knn_cache_clear(disk: bool = False) -> None:
    _TABLES.clear()
    _TREES.clear()
    for k in _cache_stats:
        _cache_stats[k] = 0
    d = knn_cache_dir()
    if disk and d:
        import glob
        import os

        for f in glob.glob(os.path.join(d, "knn-*.npz")):
            os.remove(f)


def knn_cache_info() -> dict:
    return dict(_cache_stats, tables=len(_TABLES), bytes=sum(i.nbytes + d.nbytes for i, d in _TABLES.values()), trees=len(_TREES),
                directory=knn_cache_dir())


def host_tree(src_xyz: np.ndarray, key: str | None = None):
    """``cKDTree(src_xyz)`` remembered per source point set (the build is 60 % of a query on O1280)."""
    from scipy.spatial import cKDTree

    key = key or points_hash(src_xyz)
    tree = _TREES.get(key)
    if tree is None:
        tree = cKDTree(src_xyz)
        _cache_stats["trees_built"] += 1
        _TREES[key] = tree
        while len(_TREES) > _TREES_MAX:
            _TREES.popitem(last=False)
    else:
        _TREES.move_to_end(key)
    return tree


def _remembered_table(src_lat, src_lon, tgt_lat, tgt_lon, k: int, max_distance, order: str, compute, producer: str = "host"):
    """``(indices [n, k] int64, distances [n, k] float64)`` from the process memo, the disk cache or ``compute(src_hash)``;
    the arrays handed back are the caller's own copies.

    Entries are kept per PRODUCER (``"host"``: cKDTree itself; ``"device"``: ``atx_knn_*`` with cKDTree settling the ties) and per
    ``KNN_TABLE_FORMAT``: a table the device search built is never served to the host path (or the other way round), and a
    change to the kernel's tie handling or to the file layout is a bump of that constant, which orphans the old files instead
    of trusting them.  Files also record producer, format and library version and are re-checked on load."""
    import os

    src_h, tgt_h = points_hash(src_lat, src_lon), points_hash(tgt_lat, tgt_lon)
    bound = "none" if max_distance is None else repr(float(max_distance))
    key = (src_h, tgt_h, int(k), bound, order, producer, KNN_TABLE_FORMAT)
    hit = _TABLES.get(key)
    if hit is not None:
        _TABLES.move_to_end(key)
        _cache_stats["memory_hits"] += 1
        return hit[0].copy(), hit[1].copy()
    n_src, n_tgt = int(np.size(src_lat)), int(np.size(tgt_lat))
    directory = knn_cache_dir() if n_tgt * k >= _DISK_MIN_ENTRIES else None
    path = None
    table = None
    if directory:
        path = os.path.join(directory, f"knn-v{KNN_TABLE_FORMAT}-{producer}-{order}-{src_h}-{tgt_h}-k{k}-d{bound}.npz")
        if os.path.exists(path):
            try:
                with np.load(path) as f:
                    if (tuple(f["matrix_shape"]) == (n_tgt, n_src) and f["matrix_indices"].size == n_tgt * k
                            and int(f["format"]) == KNN_TABLE_FORMAT and str(f["producer"]) == producer and str(f["tie_order"]) == order
                            and str(f["in_grid_hash"]) == src_h and str(f["out_grid_hash"]) == tgt_h):
                        table = (f["matrix_indices"].astype(np.int64).reshape(n_tgt, k), f["matrix_data"].reshape(n_tgt, k))
                        _cache_stats["disk_hits"] += 1
            except Exception:  # a damaged file is a miss (and is rewritten below)
                table = None
    if table is None:
        _cache_stats["misses"] += 1
        indices, distances = compute(src_h)
        table = (np.ascontiguousarray(indices, dtype=np.int64).reshape(n_tgt, k), np.ascontiguousarray(distances, dtype=np.float64).reshape(n_tgt, k))
        if path:
            try:
                os.makedirs(directory, exist_ok=True)
                tmp = f"{path}.{os.getpid()}.tmp.npz"
                np.savez(tmp, matrix_data=table[1].reshape(-1), matrix_indices=table[0].astype(np.int32).reshape(-1),
                         matrix_indptr=np.arange(n_tgt + 1, dtype=np.int64) * k, matrix_shape=np.array([n_tgt, n_src]),
                         kind=np.array("k-NN table: matrix_data holds chord distances on the unit sphere, not weights"),
                         in_grid_hash=np.array(src_h), out_grid_hash=np.array(tgt_h), format=np.array(KNN_TABLE_FORMAT),
                         producer=np.array(producer), tie_order=np.array(order), library_version=np.array(_library_version()))
                os.replace(tmp, path)
                global _cache_dir_announced
                if not _cache_dir_announced:
                    _cache_dir_announced = True
                    LOG.info("k-NN tables are remembered under %s (ATX_CACHE_DIR=off disables the files)", directory)
            except OSError:  # a read-only or full cache directory must not fail the filter
                pass
    _TABLES[key] = table
    total = sum(i.nbytes + d.nbytes for i, d in _TABLES.values())
    while total > _TABLES_MAX_BYTES and len(_TABLES) > 1:
        _, (i, d) = _TABLES.popitem(last=False)
        total -= i.nbytes + d.nbytes
    return table[0].copy(), table[1].copy()


def device_knn(src_xyz: np.ndarray, tgt_xyz: np.ndarray, k: int, *, ties: str = "ckdtree", max_distance: float | None = None,
               tree_key: str | None = None):
    """``(indices int64 [n, k], squared distances float64 [n, k], n_rows_resolved)`` — the k nearest rows of
    ``src_xyz`` for every row of ``tgt_xyz``, searched on the MI355X (``atx_knn_build`` / ``atx_knn_query``).

    The kernel's distances are bit-identical to cKDTree's, so its neighbour lists can differ from cKDTree's only in the
    ORDER (or, at the k-th place, the choice) of EXACTLY equidistant candidates: the kernel orders them by source index,
    cKDTree by whichever it meets first in its traversal (R: spatial.py:628 — an artefact of ``std::nth_element`` during
    its tree build, not reproducible without running that build).  ``ties="ckdtree"`` (default) makes the result
    identical to the reference's anyway: the device returns one neighbour more than asked for, rows in which two adjacent
    distances among those k+1 are equal are found on the device, and only those rows (0.14 % for O1280 -> 0.25 degree)
    are answered again by ``cKDTree(src).query`` on the host — the reference's own statement.  The host tree is built
    only if such rows exist.  ``ties="index"`` skips that and keeps the kernel's deterministic order.
    """
    import torch

    from . import native
    from . import stack as _stack

    if ties not in ("ckdtree", "index"):
        raise ValueError(f"ties must be 'ckdtree' or 'index', got {ties!r}")
    if not 1 <= k <= MAX_DEVICE_K:
        raise ValueError(f"the device k-NN search returns 1..{MAX_DEVICE_K} neighbours, got k={k}")
    dev = _stack.device()
    src_xyz = np.ascontiguousarray(src_xyz, dtype=np.float64)
    tgt_xyz = np.ascontiguousarray(tgt_xyz, dtype=np.float64)
    n_tgt = len(tgt_xyz)
    if n_tgt == 0:
        return np.zeros((0, k), dtype=np.int64), np.zeros((0, k)), 0
    ahead = 1 if ties == "ckdtree" else 0
    idx_d, d2_d = native.KnnIndex(torch.from_numpy(src_xyz).to(dev)).query(torch.from_numpy(tgt_xyz).to(dev), k + ahead)
    rows = None
    if ahead:
        # a finite distance equal to its successor: the candidates' order (or which of them is the k-th) is cKDTree's to decide
        tied = ((d2_d[:, :-1] == d2_d[:, 1:]) & torch.isfinite(d2_d[:, :-1])).any(dim=1)
        rows = torch.nonzero(tied).reshape(-1).cpu().numpy()
    indices = idx_d[:, :k].cpu().numpy().astype(np.int64)
    d2 = d2_d[:, :k].cpu().numpy()
    if rows is not None and rows.size:
        kwargs = {} if max_distance is None else {"distance_upper_bound": max_distance}
        host_d, host_i = host_tree(src_xyz, tree_key).query(tgt_xyz[rows], k=k, **kwargs)
        host_d, host_i = host_d.reshape(len(rows), k), host_i.reshape(len(rows), k)
        # cKDTree reports sqrt(d2); the squared distances are the same multiset per row, re-ordered like the indices
        found = host_i < len(src_xyz)
        diff = src_xyz[np.where(found, host_i, 0)] - tgt_xyz[rows][:, None, :]
        host_d2 = np.zeros(host_i.shape)
        for c in range(3):  # s = 0; s += dx*dx; ... — scipy's order, as in the kernel
            host_d2 = host_d2 + diff[..., c] * diff[..., c]
        indices[rows] = host_i
        d2[rows] = np.where(found, host_d2, np.inf)
    return indices, d2, 0 if rows is None else int(rows.size)


def nearest_grid_points_device(
    source_latitudes,
    source_longitudes,
    target_latitudes,
    target_longitudes,
    max_distance: float | None = None,
    num_neighbours_to_return: int = 1,
    return_distances: bool = False,
    ties: str = "ckdtree",
):
    """``nearest_grid_points`` computed on the MI355X (``atx_knn_build`` / ``atx_knn_query``).

    Same arguments and return values as R: spatial.py:587-635, and — with the default ``ties="ckdtree"`` — the same
    bits: distances are bit-identical to cKDTree's (coordinates are computed on the host exactly as the reference does,
    the kernel repeats scipy's float64 arithmetic), and rows with exactly equidistant candidates are settled by cKDTree
    itself (``device_knn``).  ``ties="index"`` orders such candidates by source index and never touches the host tree.
    """
    k = int(num_neighbours_to_return)

    def compute(src_hash):
        src = unit_sphere_xyz(source_latitudes, source_longitudes)
        tgt = unit_sphere_xyz(target_latitudes, target_longitudes)
        indices, d2, _ = device_knn(src, tgt, k, ties=ties, max_distance=max_distance, tree_key=src_hash)
        distances = np.sqrt(d2)
        if max_distance is not None:  # cKDTree: neighbours at d >= distance_upper_bound are "missing"
            missing = ~(distances < max_distance)
            indices[missing] = len(src)
            distances[missing] = np.inf
        return indices, distances

    indices, distances = _remembered_table(source_latitudes, source_longitudes, target_latitudes, target_longitudes, k, max_distance,
                                           ties, compute, producer="device")
    if k == 1:
        indices, distances = indices[:, 0], distances[:, 0]
    if return_distances:
        return indices, distances
    return indices


def nearest_grid_points(
    source_latitudes,
    source_longitudes,
    target_latitudes,
    target_longitudes,
    max_distance: float | None = None,
    num_neighbours_to_return: int = 1,
    return_distances: bool = False,
):
    """k nearest source points of every target point, by chord distance.

    Same call surface and return order as the reference (R: spatial.py:587-635):
    ``indices`` (int64, ``[Nt]`` or ``[Nt, k]``) or ``(indices, distances)``.
    With ``max_distance`` cKDTree reports ``len(source)`` for "none found"
    (R: spatial.py:630-632); the regrid filter rejects such indices before any
    gather (``native.check_indices``).
    """
    if knn_engine() == "device":
        return nearest_grid_points_device(
            source_latitudes, source_longitudes, target_latitudes, target_longitudes, max_distance=max_distance,
            num_neighbours_to_return=num_neighbours_to_return, return_distances=return_distances,
        )
    k = int(num_neighbours_to_return)

    def compute(src_hash):
        tree = host_tree(unit_sphere_xyz(source_latitudes, source_longitudes), src_hash)
        kwargs = {} if max_distance is None else {"distance_upper_bound": max_distance}
        distances, indices = tree.query(unit_sphere_xyz(target_latitudes, target_longitudes), k=k, **kwargs)
        return indices, distances

    indices, distances = _remembered_table(source_latitudes, source_longitudes, target_latitudes, target_longitudes, k, max_distance,
                                           "ckdtree", compute)
    if k == 1:  # cKDTree's own shapes: [Nt] for k = 1, [Nt, k] otherwise
        indices, distances = indices[:, 0], distances[:, 0]
    if return_distances:
        return indices, distances
    return indices


def knn_inverse_distance(in_grid: dict, out_grid: dict, k: int = 4, floor: float = 1e-12, device: bool = False,
                         ties: str = "ckdtree"):
    """k-NN inverse-distance weights ``w_j = (1/max(d_j, floor)) / sum``.

    Returns ``(idx [Nt, k] int64, w [Nt, k] float64)``.  ``device=True`` runs the neighbour
    search on the GPU (``nearest_grid_points_device``; ``ties`` as there) instead of cKDTree.
    """
    kwargs = dict(ties=ties) if device else {}
    search = nearest_grid_points_device if device else nearest_grid_points
    idx, dist = search(
        in_grid["latitudes"], in_grid["longitudes"], out_grid["latitudes"], out_grid["longitudes"],
        num_neighbours_to_return=k, return_distances=True, **kwargs,
    )
    idx = idx.reshape(len(idx), -1)
    dist = dist.reshape(len(dist), -1)
    inv = 1.0 / np.maximum(dist, floor)
    return idx, inv / inv.sum(axis=1, keepdims=True)


def ell_to_csr(idx: np.ndarray, w: np.ndarray, n_src: int) -> dict[str, np.ndarray]:
    """Fixed-k index/weight table as the CSR triplet of the MIR npz format."""
    n_tgt, k = idx.shape
    return dict(
        matrix_data=np.ascontiguousarray(w, dtype=np.float64).reshape(-1),
        matrix_indices=np.ascontiguousarray(idx, dtype=np.int32).reshape(-1),
        matrix_indptr=(np.arange(n_tgt + 1, dtype=np.int64) * k).astype(np.int32),
        matrix_shape=np.array([n_tgt, n_src]),
    )


def csr_uniform_k(indptr: np.ndarray) -> int | None:
    """Row length if every CSR row holds the same number of entries, else ``None``."""
    lengths = np.diff(indptr)
    if lengths.size and (lengths == lengths[0]).all() and lengths[0] > 0:
        return int(lengths[0])
    return None


def bilinear_rows(row_latitudes: np.ndarray, row_lengths: np.ndarray, out_grid: dict) -> dict[str, np.ndarray]:
    """Bilinear weights from a ROW-STRUCTURED global grid (rows of constant latitude, north to south, row ``r`` holding
    ``row_lengths[r]`` equally spaced longitudes starting at 0 — octahedral / classic reduced / full Gaussian and regular
    lat-lon grids) to arbitrary target points.

    Two bracketing rows x two bracketing longitudes per row (periodic), linear in longitude on each row, then linear in
    latitude; above the first / below the last row the nearest row is used alone.  Always 4 entries per target (zero
    weights are kept) so the matrix is fixed-k.
    """
    lats = np.asarray(row_latitudes, dtype=np.float64)  # north -> south
    nlon = np.asarray(row_lengths, dtype=np.int64)
    if lats.ndim != 1 or lats.shape != nlon.shape or len(lats) < 1 or np.any(np.diff(lats) >= 0) or np.any(nlon < 1):
        raise ValueError("rows must be given north to south with strictly decreasing latitudes and positive lengths")
    row_start = np.concatenate([[0], np.cumsum(nlon)[:-1]])
    tlat = np.asarray(out_grid["latitudes"], dtype=np.float64)
    tlon = np.mod(np.asarray(out_grid["longitudes"], dtype=np.float64), 360.0)

    # first row whose latitude is <= target latitude (rows descend)
    south = np.searchsorted(-lats, -tlat, side="left")
    north = south - 1
    south = np.clip(south, 0, len(lats) - 1)
    north = np.clip(north, 0, len(lats) - 1)
    span = lats[north] - lats[south]
    w_north = np.where(span > 0, (tlat - lats[south]) / np.where(span > 0, span, 1.0), 1.0)
    w_north = np.clip(w_north, 0.0, 1.0)

    idx = np.empty((len(tlat), 4), dtype=np.int64)
    w = np.empty((len(tlat), 4), dtype=np.float64)
    for slot, (row, w_row) in enumerate(((north, w_north), (south, 1.0 - w_north))):
        m = nlon[row]
        x = tlon * (m / 360.0)
        j0 = np.floor(x).astype(np.int64)
        frac = x - j0
        j0 = np.mod(j0, m)
        j1 = np.mod(j0 + 1, m)
        idx[:, 2 * slot] = row_start[row] + j0
        idx[:, 2 * slot + 1] = row_start[row] + j1
        w[:, 2 * slot] = w_row * (1.0 - frac)
        w[:, 2 * slot + 1] = w_row * frac
    return ell_to_csr(idx, w, int(nlon.sum()))


def bilinear_octahedral(n: int, out_grid: dict) -> dict[str, np.ndarray]:
    """``bilinear_rows`` from the octahedral grid ``O<n>`` (BASELINE config 2: O96 -> 1 degree)."""
    return bilinear_rows(gaussian_latitudes(2 * n), octahedral_row_lengths(n), out_grid)


def box_row_table(rows: tuple[np.ndarray, np.ndarray]) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(z, lengths, starts)`` of a row-structured grid's CELLS: ``z`` float64 ``[R + 1]`` is the sine of the rows' latitude edges
    (90, the midpoints between adjacent row latitudes, -90), descending, with ``z[0] = 1`` and ``z[R] = -1`` set exactly; ``lengths``
    int64 ``[R]``; ``starts`` int64 ``[R + 1]`` (``starts[R]`` is the number of points).  Rows that do not descend strictly or hold
    fewer than 2 points raise ``ValueError``."""
    lats = np.asarray(rows[0], dtype=np.float64)
    lengths = np.asarray(rows[1])
    if lats.ndim != 1 or lats.shape != lengths.shape or len(lats) < 1 or lengths.dtype.kind not in "iu":
        raise ValueError("a row structure is (row latitudes [R], integer row lengths [R]) with R >= 1")
    lengths = lengths.astype(np.int64)
    if np.any(np.diff(lats) >= 0) or lats[0] > 90.0 or lats[-1] < -90.0:
        raise ValueError("rows must be given north to south with strictly decreasing latitudes within [-90, 90]")
    if np.any(lengths < 2):
        raise ValueError("grid-box averaging needs at least 2 points in every row")
    edges = np.concatenate([[90.0], 0.5 * (lats[:-1] + lats[1:]), [-90.0]])
    z = np.sin(np.deg2rad(edges))
    z[0], z[-1] = 1.0, -1.0
    if np.any(np.diff(z) >= 0):  # a pole row AT the pole is a half-height cell; two rows there would be a cell of no height
        raise ValueError("the latitude edges of the rows do not descend strictly")
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    if starts[-1] >= 2**31:
        raise NotImplementedError("grids with 2^31 or more points are not supported")
    return z, lengths, starts


def _sequential_row_sums(raw: np.ndarray, indptr: np.ndarray) -> np.ndarray:
    """Sum of every CSR row accumulated from 0 in the order of its entries (``np.add.reduceat`` may add pairwise)."""
    counts = np.diff(indptr)
    tot = np.zeros(len(counts), dtype=np.float64)
    first = indptr[:-1]
    for k in range(int(counts.max()) if counts.size else 0):
        live = np.flatnonzero(counts > k)
        tot[live] += raw[first[live] + k]
    return tot


def box_average_rows(src_rows: tuple[np.ndarray, np.ndarray], tgt_rows: tuple[np.ndarray, np.ndarray], *,
                     device: bool = False) -> dict[str, np.ndarray]:
    """Grid-box-average (first-order conservative) weights between two ROW-STRUCTURED global grids, each given as
    ``(row latitudes north to south, points per row)`` (``grids.row_structure``): the value of a target cell is the mean of the
    source cells under it, weighted by the area they share.

    Cells.  Row ``r`` spans the latitude edges ``e_r .. e_{r+1}``: ``e_0 = 90``, ``e_R = -90``, midpoints between row latitudes
    otherwise; ``z = sin(deg2rad(e))`` in float64 here on the host, ``z_0 = 1`` and ``z_R = -1`` exactly (``box_row_table``).  Cell
    ``j`` of a row of ``n`` is the arc ``[(j - 1/2) 360/n, (j + 1/2) 360/n)``; cell 0 straddles 0 degrees.

    Latitude.  ``dz = min(zt[r], zs[q]) - max(zt[r+1], zs[q+1])``; source row ``q`` takes part in target row ``r`` iff
    ``dz > 2**-40 * (zt[r] - zt[r+1])`` (edges of aligned lat-lon pairs that are equal in exact arithmetic differ in the last
    bit; such slivers are ~1e-14 of a row, real overlaps are at least 1 / (row ratio)).

    Longitude.  In units of ``360 / (2 ns nt)`` degrees the edges of target cell ``i`` (of ``nt``) and source cell ``j`` (of ``ns``)
    are the integers ``(2i -+ 1) ns`` and ``(2j -+ 1) nt`` modulo ``2 ns nt``; ``ov`` is the length of the arcs' intersection, an
    exact int64 including the wrap.  The entry exists iff ``ov > 0``.

    Weights.  ``raw = dz * (float(ov) / float(2 ns nt))``; the entries of a target are kept in ascending source index, ``tot`` is
    their sum accumulated from 0 in that order, ``w = raw / tot``.

    Returns the CSR triplet of the MIR npz format, as ``ell_to_csr`` does.  ``device=False`` evaluates the statement in numpy;
    ``device=True`` runs ``atx_plan_box_average_count`` / ``_fill`` (``include/atx_plan.h``) and returns the same arrays bit
    for bit.  2^31 or more entries raise ``NotImplementedError``.
    """
    zs, slen, sstart = box_row_table(src_rows)
    zt, tlen, tstart = box_row_table(tgt_rows)
    n_src, n_tgt = int(sstart[-1]), int(tstart[-1])
    if device:
        return _box_average_device((zs, slen, sstart), (zt, tlen, tstart))

    targets, columns, raws = [], [], []
    for r in range(len(tlen)):
        top, bot, nt = zt[r], zt[r + 1], int(tlen[r])
        dz_rows = np.minimum(top, zs[:-1]) - np.maximum(bot, zs[1:])
        i = np.arange(nt, dtype=np.int64)
        row_t, row_c, row_w = [], [], []
        for q in np.flatnonzero(dz_rows > 2.0**-40 * (top - bot)):
            ns = int(slen[q])
            a, b = (2 * i - 1) * ns, (2 * i + 1) * ns
            jlo = (a - nt) // (2 * nt) + 1  # the first source cell whose east edge lies east of the target's west edge ...
            count = (b + nt - 1) // (2 * nt) - jlo + 1  # ... to the last whose west edge lies west of the target's east edge
            cell = np.repeat(i, count)
            ju = np.repeat(jlo, count) + (np.arange(int(count.sum()), dtype=np.int64) - np.repeat(np.cumsum(count) - count, count))
            ov = np.minimum(b[cell], (2 * ju + 1) * nt) - np.maximum(a[cell], (2 * ju - 1) * nt)
            row_t.append(cell)
            row_c.append(sstart[q] + np.mod(ju, ns))
            row_w.append(dz_rows[q] * (ov.astype(np.float64) / float(2 * ns * nt)))
        if row_t:
            cell, column, raw = np.concatenate(row_t), np.concatenate(row_c), np.concatenate(row_w)
            order = np.lexsort((column, cell))  # by target, ascending source index within it (a wrapped run's j = 0 ... part first)
            targets.append(tstart[r] + cell[order])
            columns.append(column[order])
            raws.append(raw[order])
    target = np.concatenate(targets) if targets else np.zeros(0, dtype=np.int64)
    column = np.concatenate(columns) if columns else np.zeros(0, dtype=np.int64)
    raw = np.concatenate(raws) if raws else np.zeros(0, dtype=np.float64)
    if len(raw) >= 2**31:
        raise NotImplementedError("matrices with 2^31 or more entries are not supported")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(target, minlength=n_tgt))]).astype(np.int64)
    tot = _sequential_row_sums(raw, indptr)
    return dict(
        matrix_data=raw / np.repeat(tot, np.diff(indptr)),
        matrix_indices=column.astype(np.int32),
        matrix_indptr=indptr.astype(np.int32),
        matrix_shape=np.array([n_tgt, n_src]),
    )


def _box_average_device(src: tuple[np.ndarray, np.ndarray, np.ndarray], tgt: tuple[np.ndarray, np.ndarray, np.ndarray]) -> dict[str, np.ndarray]:
    """``box_average_rows`` on the current device: count, scan (``torch.cumsum``), fill.  The tables were validated by ``box_row_table``."""
    import torch

    from . import native_plan

    if not torch.cuda.is_available():
        raise RuntimeError("box_average_rows(device=True) needs a GPU; device=False evaluates the same statement on the host")
    dev = torch.device("cuda", torch.cuda.current_device())
    tables = [native_plan.RowTable(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in t), n_points=int(t[2][-1])) for t in (src, tgt)]
    n_src, n_tgt = tables[0].n_points, tables[1].n_points
    count = torch.empty(n_tgt, dtype=torch.int64, device=dev)
    native_plan.box_average_count(tables[0], tables[1], count)
    ends = torch.cumsum(count, dim=0)
    nnz = int(ends[-1].item())
    if nnz >= 2**31:
        raise NotImplementedError("matrices with 2^31 or more entries are not supported")
    indptr = torch.zeros(n_tgt + 1, dtype=torch.int32, device=dev)
    indptr[1:] = ends.to(torch.int32)
    indices = torch.empty(nnz, dtype=torch.int32, device=dev)
    data = torch.empty(nnz, dtype=torch.float64, device=dev)
    native_plan.box_average_fill(tables[0], tables[1], indptr, indices, data)
    return dict(matrix_data=data.cpu().numpy(), matrix_indices=indices.cpu().numpy(), matrix_indptr=indptr.cpu().numpy(),
                matrix_shape=np.array([n_tgt, n_src]))


# ---- linear interpolation from any set of source points: triangulate, locate, three barycentric weights ---------------------------
SLIVER = 2.0**-20  # a triangle with det(v0, v1, v2) < SLIVER * (longest edge)^2 is not part of the domain
INSIDE = 2.0**-30  # a target is inside a triangle when every d_i >= -INSIDE * D
FOUND, UNDECIDED, OUTSIDE, MALFORMED = 0, 1, 2, 3  # the status codes of the walk (include/atx_mesh.h)
WALK_STEPS = 64  # moves a target is given before brute force decides it


def _det(p: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """``p.x (b.y c.z - b.z c.y) + p.y (b.z c.x - b.x c.z) + p.z (b.x c.y - b.y c.x)`` over the last axis: every operation rounded on
    its own, the sum taken left to right — the expression of ``atx_mesh_locate``."""
    cx = b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]
    cy = b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2]
    cz = b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]
    return (p[..., 0] * cx + p[..., 1] * cy) + p[..., 2] * cz


def triangulate_sphere(src_xyz: np.ndarray, max_edge: float | None = None) -> dict[str, np.ndarray]:
    """The spherical Delaunay triangulation of unit vectors ``src_xyz`` (float64 ``[n, 3]``): the convex hull of points on the unit
    sphere, from ``scipy.spatial.ConvexHull`` (Qhull).  Returns

    - ``tri`` int32 ``[T, 3]``, every triangle oriented so that ``det(v0, v1, v2) > 0`` (where Qhull's is not, vertices 1 and 2
      are swapped, and the neighbour columns 1 and 2 with them);
    - ``nbr`` int32 ``[T, 3]``: ``nbr[t, e]`` is the triangle across the edge opposite vertex ``e``;
    - ``flag`` uint8 ``[T]``: with ``L`` the longest chord edge and ``D = det(v0, v1, v2)``, set where ``D < 2^-20 L^2`` (slivers:
      collinear boundary points of a lat-lon box) or where ``max_edge`` is given and ``L > max_edge`` (the faces that close the
      hull around a limited-area domain);
    - ``hull_vertices`` int64, sorted: the points that are a vertex of some triangle.  The others (duplicates, such as the surplus
      pole points of a lat-lon grid) carry no weight;
    - ``vertex_tri`` int32 ``[n]``: the lowest-numbered unflagged triangle at the vertex, else the lowest flagged one, -1 for a
      point that is no hull vertex.

    Non-finite coordinates, fewer than four points and a degenerate hull raise ``ValueError``.
    """
    from scipy.spatial import ConvexHull, QhullError

    xyz = np.ascontiguousarray(src_xyz, dtype=np.float64)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"source points must be unit vectors [n, 3], got shape {xyz.shape}")
    if not np.isfinite(xyz).all():
        raise ValueError("source coordinates must be finite")
    n = len(xyz)
    if n < 4:
        raise ValueError(f"a triangulation needs at least four source points, got {n}")
    if n >= 2**31:
        raise NotImplementedError("grids with 2^31 or more points are not supported")
    try:
        hull = ConvexHull(xyz)
    except QhullError as e:
        raise ValueError(f"the source points have no triangulation (degenerate hull): {str(e).strip().splitlines()[0]}") from None
    tri = hull.simplices.astype(np.int32)
    nbr = hull.neighbors.astype(np.int32)
    if len(tri) < 4 or (nbr < 0).any():
        raise ValueError("the source points have no triangulation (degenerate hull)")
    swap = ~(_det(xyz[tri[:, 0]], xyz[tri[:, 1]], xyz[tri[:, 2]]) > 0.0)
    tri[swap] = tri[swap][:, [0, 2, 1]]
    nbr[swap] = nbr[swap][:, [0, 2, 1]]
    v0, v1, v2 = xyz[tri[:, 0]], xyz[tri[:, 1]], xyz[tri[:, 2]]
    det = _det(v0, v1, v2)
    longest2 = np.max([np.sum((v1 - v2) ** 2, axis=1), np.sum((v2 - v0) ** 2, axis=1), np.sum((v0 - v1) ** 2, axis=1)], axis=0)
    flag = det < SLIVER * longest2
    if max_edge is not None:
        flag |= np.sqrt(longest2) > float(max_edge)
    number = np.repeat(np.arange(len(tri), dtype=np.int64), 3)
    corner = tri.reshape(-1).astype(np.int64)
    lowest = np.full((2, n), len(tri), dtype=np.int64)  # per vertex: the lowest unflagged, the lowest flagged triangle
    flagged = np.repeat(flag, 3)
    np.minimum.at(lowest[0], corner[~flagged], number[~flagged])
    np.minimum.at(lowest[1], corner[flagged], number[flagged])
    vertex_tri = np.where(lowest[0] < len(tri), lowest[0], np.where(lowest[1] < len(tri), lowest[1], -1)).astype(np.int32)
    return dict(tri=np.ascontiguousarray(tri), nbr=np.ascontiguousarray(nbr), flag=flag.astype(np.uint8),
                hull_vertices=np.flatnonzero(vertex_tri >= 0), vertex_tri=vertex_tri)


def _weights(d: np.ndarray) -> np.ndarray:
    """``w_i = d_i / ((d0 + d1) + d2)`` with negative ``d_i`` clamped to 0, for ``d`` float64 ``[n, 3]``: the barycentric coordinates
    of the point where the ray through the target meets the triangle's plane."""
    d = np.where(d < 0.0, 0.0, d)
    return d / ((d[:, 0] + d[:, 1]) + d[:, 2])[:, None]


def locate_walk_host(src_xyz, tri, nbr, flag, tgt_xyz, seed, max_steps: int = 64):
    """Walk every target from its seed triangle to the triangle under it, vectorised over the targets still walking; the statement
    that ``atx_mesh_locate`` repeats operation for operation.  Returns ``(tri_out int32 [n], w float64 [n, 3], status int32 [n],
    steps int32 [n])``.  At triangle ``t = (a, b, c)`` and target ``p``:

    1. ``flag[t]`` set: status 2 (outside), stop.
    2. ``d0 = det(p, b, c)``, ``d1 = det(p, c, a)``, ``d2 = det(p, a, b)``, ``D = det(a, b, c)`` (``_det``).
    3. every ``d_i >= -2^-30 D``: status 0 (found), ``w`` from ``_weights``.
    4. ``max_steps`` moves made already: status 1 (undecided), stop.
    5. move to ``nbr[t, e]``, ``e`` the first of the smallest ``d_i`` (``np.argmin``'s choice).

    ``tri_out`` is the triangle at which the target stopped.  A seed or neighbour outside ``[0, T)`` or a vertex outside
    ``[0, n_src)`` ends the target with status 3, ``tri_out`` -1 and NaN weights; ``w`` is 0 with status 1 and 2.
    """
    xyz = np.asarray(src_xyz, dtype=np.float64)
    tgt = np.asarray(tgt_xyz, dtype=np.float64)
    tri, nbr, flag = np.asarray(tri), np.asarray(nbr), np.asarray(flag)
    n, n_tri, n_src = len(tgt), len(tri), len(xyz)
    current = np.asarray(seed).astype(np.int64).copy()
    w = np.zeros((n, 3), dtype=np.float64)
    status = np.full(n, UNDECIDED, dtype=np.int32)
    steps = np.zeros(n, dtype=np.int32)
    active = np.arange(n, dtype=np.int64)

    def stop(rows, code):
        status[rows] = code
        if code == MALFORMED:
            current[rows], w[rows] = -1, np.nan

    while active.size:
        t = current[active]
        ok = (t >= 0) & (t < n_tri)
        stop(active[~ok], MALFORMED)
        active, t = active[ok], t[ok]
        inside = flag[t] == 0
        stop(active[~inside], OUTSIDE)
        active, t = active[inside], t[inside]
        corners = tri[t].astype(np.int64)
        ok = ((corners >= 0) & (corners < n_src)).all(axis=1)
        stop(active[~ok], MALFORMED)
        active, t, corners = active[ok], t[ok], corners[ok]
        p, a, b, c = tgt[active], xyz[corners[:, 0]], xyz[corners[:, 1]], xyz[corners[:, 2]]
        d = np.stack([_det(p, b, c), _det(p, c, a), _det(p, a, b)], axis=1)
        tol = -INSIDE * _det(a, b, c)
        found = (d[:, 0] >= tol) & (d[:, 1] >= tol) & (d[:, 2] >= tol)
        w[active[found]] = _weights(d[found])
        stop(active[found], FOUND)
        active, t, d = active[~found], t[~found], d[~found]
        spent = steps[active] >= max_steps
        stop(active[spent], UNDECIDED)
        active, t, d = active[~spent], t[~spent], d[~spent]
        edge = np.where(d[:, 1] < d[:, 0], 1, 0)  # strict comparisons: the first of equal minima stays
        edge = np.where(d[:, 2] < np.where(edge == 1, d[:, 1], d[:, 0]), 2, edge)
        current[active] = nbr[t, edge]
        steps[active] += 1
    return current.astype(np.int32), w, status, steps


def locate_brute_host(src_xyz, tri, flag, tgt_xyz, chunk: int = 256):
    """The triangle under every target without a walk: of the unflagged triangles the one with the largest ``min_i d_i / D``, the
    lowest-numbered on ties; the target is inside (status 0) iff that value is ``>= -2^-30``, with the clamp and the weights of
    ``locate_walk_host``, and outside (status 2, ``tri_out`` -1, weights 0) otherwise.  Returns ``(tri_out int32 [n], w float64
    [n, 3], status int32 [n])``.  Targets are taken ``chunk`` at a time, fewer on a large mesh: O(chunk * T) memory, 2^22 values at most."""
    xyz = np.asarray(src_xyz, dtype=np.float64)
    tgt = np.asarray(tgt_xyz, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(tri)
    n = len(tgt)
    tri_out = np.full(n, -1, dtype=np.int32)
    w = np.zeros((n, 3), dtype=np.float64)
    status = np.full(n, OUTSIDE, dtype=np.int32)
    keep = np.flatnonzero(np.asarray(flag) == 0)
    if keep.size == 0 or n == 0:
        return tri_out, w, status
    a, b, c = (xyz[tri[keep, i]] for i in range(3))
    det_abc = _det(a, b, c)
    # det(p, b, c) = (p.x X.x + p.y X.y) + p.z X.z with X = b x c rounded as in _det: the same bits, X computed once per triangle
    crosses = [np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]])
               for u, v in ((b, c), (c, a), (a, b))]
    chunk = max(1, min(int(chunk), (1 << 22) // len(keep)))  # at most 2^22 determinants (32 MiB) per temporary
    for lo in range(0, n, chunk):
        p = tgt[lo:lo + chunk]
        least = None
        for x in crosses:
            d = (p[:, 0:1] * x[0] + p[:, 1:2] * x[1]) + p[:, 2:3] * x[2]
            least = d if least is None else np.minimum(least, d)
        least /= det_abc
        best = np.argmax(least, axis=1)  # the first of equal maxima: the lowest-numbered triangle
        rows = np.flatnonzero(least[np.arange(len(p)), best] >= -INSIDE)
        t = keep[best[rows]]
        q, ta, tb, tc = p[rows], xyz[tri[t, 0]], xyz[tri[t, 1]], xyz[tri[t, 2]]
        tri_out[lo + rows] = t
        w[lo + rows] = _weights(np.stack([_det(q, tb, tc), _det(q, tc, ta), _det(q, ta, tb)], axis=1))
        status[lo + rows] = FOUND
    return tri_out, w, status


def _nearest_by_index(src_xyz: np.ndarray, tgt_xyz: np.ndarray) -> np.ndarray:
    """The nearest row of ``src_xyz`` for every target, the lowest-numbered of exactly equidistant ones — what ``device_knn(k=1,
    ties="index")`` returns.  cKDTree finds the candidates; squared distances are summed in its (and the kernel's) order."""
    from scipy.spatial import cKDTree

    tree = cKDTree(src_xyz)
    k = min(2, len(src_xyz))
    dist, idx = tree.query(tgt_xyz, k=k)
    dist, idx = dist.reshape(len(tgt_xyz), k), idx.reshape(len(tgt_xyz), k).astype(np.int64)
    nearest = idx[:, 0].copy()
    if k == 2:
        for row in np.flatnonzero(dist[:, 1] <= dist[:, 0] * (1.0 + 2.0**-40) + 2.0**-500):  # a possible tie: look at every candidate
            near = np.sort(np.asarray(tree.query_ball_point(tgt_xyz[row], dist[row, 1] * (1.0 + 2.0**-40) + 2.0**-500), dtype=np.int64))
            diff = src_xyz[near] - tgt_xyz[row]
            d2 = np.zeros(len(near))
            for axis in range(3):
                d2 = d2 + diff[:, axis] * diff[:, axis]
            nearest[row] = near[np.argmin(d2)]  # the first of equal minima: the lowest index
    return nearest


def _grid_xyz(grid: dict, what: str) -> np.ndarray:
    lat, lon = np.asarray(grid["latitudes"], dtype=np.float64).reshape(-1), np.asarray(grid["longitudes"], dtype=np.float64).reshape(-1)
    if lat.shape != lon.shape:
        raise ValueError(f"{what}: latitudes and longitudes differ in length ({lat.shape[0]} and {lon.shape[0]})")
    if not (np.isfinite(lat).all() and np.isfinite(lon).all()):
        raise ValueError(f"{what}: coordinates must be finite")
    return np.ascontiguousarray(unit_sphere_xyz(lat, lon))  # row-major [n, 3], as the kernels read it


def linear_triangulated(in_grid: dict, out_grid: dict, *, max_edge_km: float | None = None, outside: str = "raise",
                        device: bool = False, max_steps: int = WALK_STEPS) -> dict[str, np.ndarray]:
    """Linear interpolation weights from ANY set of source points (a limited-area grid, ICON, scattered points, a dict of
    coordinates) to the target points: the source points are triangulated on the sphere (``triangulate_sphere``) and every target
    gets the three barycentric weights of the triangle under it (``locate_walk_host``) — the construction of MIR's ``linear``
    method.  Returns the CSR triplet of the MIR npz format with three entries per row, as ``ell_to_csr`` does.

    ``max_edge_km`` takes triangles with a longer edge out of the domain: without it the long faces that close the hull around a
    limited-area grid count as part of it, and targets well outside the grid get weights from them.  Targets outside the domain raise ``ValueError`` with their count
    (``outside="raise"``) or get the nearest source point with weight 1 and two entries of weight 0 (``outside="nearest"``).

    Each walk starts at ``vertex_tri`` of the nearest hull vertex (the lowest-numbered of equidistant ones) and is given
    ``max_steps`` moves; targets still undecided after ``WALK_STEPS`` (64) moves are answered by ``locate_brute_host``.  A smaller
    ``max_steps`` only bounds the first pass: its undecided rows resume the host walk where they stopped, up to 64 moves in all, so
    the matrix does not depend on ``max_steps <= 64`` (the walk is a function of the triangle it stands on; brute force may name the
    triangle on the other side of an edge that the target lies on).  ``device=True`` uploads the mesh once and runs the neighbour
    search (``atx_knn_*``, as ``device_knn(ties="index")``) and the first pass (``atx_mesh_locate``, ``include/atx_mesh.h``) on the
    GPU; only the undecided rows come back to the host statement.  The arrays are the same bit for bit either way.  The hull itself
    is always built on the host, in Qhull.
    """
    if outside not in ("raise", "nearest"):
        raise ValueError(f"outside must be 'raise' or 'nearest', got {outside!r}")
    src_xyz, tgt_xyz = _grid_xyz(in_grid, "in_grid"), _grid_xyz(out_grid, "out_grid")
    max_edge = None
    if max_edge_km is not None:
        from .spatial import R_earth_km

        if not max_edge_km > 0:
            raise ValueError(f"max_edge_km must be positive, got {max_edge_km!r}")
        max_edge = 2.0 * np.sin(min(float(max_edge_km) / R_earth_km, np.pi) / 2.0)  # the chord of that arc on the unit sphere
    mesh = triangulate_sphere(src_xyz, max_edge)
    tri, hull_vertices = mesh["tri"], mesh["hull_vertices"]
    n_src, n_tgt = len(src_xyz), len(tgt_xyz)
    if device:
        tri_out, w, status = _locate_device(src_xyz, mesh, tgt_xyz, max_steps)
    else:
        seed = mesh["vertex_tri"][hull_vertices[_nearest_by_index(src_xyz[hull_vertices], tgt_xyz)]] if n_tgt else np.zeros(0, dtype=np.int32)
        tri_out, w, status, _ = locate_walk_host(src_xyz, tri, mesh["nbr"], mesh["flag"], tgt_xyz, seed, max_steps)
    undecided = np.flatnonzero(status == UNDECIDED)
    if undecided.size and max_steps < WALK_STEPS:  # a bounded first pass: the walk goes on from where it stopped
        tri_out[undecided], w[undecided], status[undecided], _ = locate_walk_host(
            src_xyz, tri, mesh["nbr"], mesh["flag"], tgt_xyz[undecided], tri_out[undecided], WALK_STEPS - max_steps)
        undecided = np.flatnonzero(status == UNDECIDED)
    if undecided.size:
        tri_out[undecided], w[undecided], status[undecided] = locate_brute_host(src_xyz, tri, mesh["flag"], tgt_xyz[undecided])
    if (status == MALFORMED).any():
        raise RuntimeError("the walk left the triangulation: triangulate_sphere returned an inconsistent mesh")
    indices = tri[np.where(status == FOUND, tri_out, 0)].astype(np.int32)
    lost = np.flatnonzero(status != FOUND)
    if lost.size:
        if outside == "raise":
            raise ValueError(f"{lost.size} of {n_tgt} target points lie outside the triangulated source domain; give max_edge_km a "
                             "larger value (or none), or pass outside='nearest' to give them the nearest source point")
        nearest = _nearest_by_index(src_xyz, tgt_xyz[lost])
        indices[lost] = nearest[:, None]
        w[lost] = [1.0, 0.0, 0.0]
    return ell_to_csr(indices, w, n_src)


def _locate_device(src_xyz: np.ndarray, mesh: dict[str, np.ndarray], tgt_xyz: np.ndarray, max_steps: int):
    """Seeds and walk of ``linear_triangulated`` on the current device: ``(tri_out, w, status)`` as numpy arrays."""
    import torch

    from . import native, native_mesh

    if not torch.cuda.is_available():
        raise RuntimeError("linear_triangulated(device=True) needs a GPU; device=False evaluates the same statement on the host")
    n_tgt = len(tgt_xyz)
    if n_tgt == 0:
        return np.zeros(0, dtype=np.int32), np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
    dev = torch.device("cuda", torch.cuda.current_device())
    hull_vertices = mesh["hull_vertices"]
    src_d, tgt_d = torch.from_numpy(src_xyz).to(dev), torch.from_numpy(np.ascontiguousarray(tgt_xyz)).to(dev)
    hull_d = torch.from_numpy(hull_vertices).to(dev)
    nearest, _ = native.KnnIndex(src_d[hull_d].contiguous()).query(tgt_d, 1)  # equidistant candidates by index (device_knn, ties="index")
    seed = torch.from_numpy(mesh["vertex_tri"]).to(dev)[hull_d[nearest[:, 0].long()]].contiguous()
    on_device = native_mesh.Mesh(src_d, *(torch.from_numpy(mesh[name]).to(dev) for name in ("tri", "nbr", "flag")))
    tri_out, w, status, _ = native_mesh.locate(on_device, tgt_d, seed, max_steps)
    return tri_out.cpu().numpy(), w.cpu().numpy(), status.cpu().numpy()


def save_matrix_npz(path: str, matrix: dict[str, np.ndarray], in_grid: dict, out_grid: dict) -> None:
    """Write the regrid-matrix npz the reference reads (R: make-regrid-file.py:150-160)."""
    np.savez(
        path,
        matrix_data=matrix["matrix_data"],
        matrix_indices=matrix["matrix_indices"],
        matrix_indptr=matrix["matrix_indptr"],
        matrix_shape=matrix["matrix_shape"],
        in_latitudes=in_grid["latitudes"],
        in_longitudes=in_grid["longitudes"],
        out_latitudes=out_grid["latitudes"],
        out_longitudes=out_grid["longitudes"],
    )


def load_matrix_npz(path: str) -> dict[str, Any]:
    """R: regrid.py:281."""
    return dict(np.load(path))
