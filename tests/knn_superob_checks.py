"""The checks that hold the k-NN, cutout and superob kernels (csrc/atx_knn.hip: ``atx_knn_build``, ``atx_knn_query``,
``atx_cutout_inside``; csrc/atx_superob.hip: ``atx_obs_group_mean``, ``atx_obs_group_argmin``) to exact host statements — written
once, as plain functions over the callables under test and a device.  tests/test_gpu_knn_superob_edges.py runs them on ``native.*``
on an MI355X; tests/test_knn_superob_checks_catch_defects.py runs them on the CPU against a numpy stand-in, once as it is and once
per planted defect.

Every comparison is equality of integers or of bit patterns, over every element of every row; no tolerance appears.  The one thing
bit patterns do not fix is WHICH NaN a missing result is (the kernel writes its own quiet NaN for an empty group, ``inf - inf`` has
the sign the machine gives it): two NaNs compare equal, everything else by bits.

The references, all independent of the package:
  k-NN    brute force in float64 with scipy's operation order (``s = 0; s += dx*dx; s += dy*dy; s += dz*dz``), candidates ordered by
          ``np.lexsort((index, s))`` — the kernel's own contract: (distance, source index) — padded with index ``n_src`` and distance
          ``+inf`` when ``k > n_src``.
  cutout  Möller–Trumbore as the kernel states it: cross products are rounded products and differences, a 3-element dot is
          ``fma(a2, b2, fma(a1, b1, a0 * b0))``; each fma is computed in rational arithmetic and rounded once (``float(Fraction)`` is
          correctly rounded).  No ``np.dot``: its rounding is the BLAS's of the machine that runs the test.
  mean    the scalar Kahan loop of tests/superob_restatement.py, one group at a time or many at once.
  argmin  a Python loop with a strict ``<`` in row order; the first non-NaN value is taken even when it is +inf; an all-NaN group
          gives its first row.

A lone ``-0.0`` in a group: the Kahan loop starts from ``sum = +0.0`` and ``+0.0 + -0.0`` is ``+0.0``, so pandas' mean of that group is
``+0.0``; the check compares the kernel's bits with that.

The edge sizes are derived from the kernels' constants, read from the sources below at import time.
"""

from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass
from fractions import Fraction
from typing import Callable, Optional

import numpy as np
import torch

from anemoi_transform_amd import native
from superob_restatement import kahan_mean, kahan_means_of_many

NAN, INF = float("nan"), float("inf")


# ---- the kernels' constants ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Constants:
    leaf: int        # kLeaf: source points per leaf bucket
    max_k: int       # kMaxK: the largest neighbour count (template instances 1 .. kMaxK)
    unroll: int      # kSuperobUnroll: rows a lane takes at a time
    long_group: int  # kLongGroup: rows from which a wave takes a group
    block: int       # kBlock
    wave: int        # kWave
    build_grid: int  # workgroup cap of blocks_for: the grid-stride build kernels

    @property
    def build_sweep(self) -> int:
        """Items one sweep of a capped build kernel takes."""
        return self.build_grid * self.block

    def past_cap_sources(self) -> int:
        """Source points whose padded leaves take four sweeps of the leaf loop and whose first merge level takes two."""
        return 2 * self.leaf * self.build_sweep + self.leaf + 1


def read_constants() -> Constants:
    csrc = os.path.join(os.path.dirname(os.path.abspath(native.__file__)), "csrc")

    def find(name, pattern):
        with open(os.path.join(csrc, name)) as f:
            m = re.search(pattern, f.read())
        assert m, f"{name}: {pattern} not found"
        return int(m.group(1))

    return Constants(
        leaf=find("atx_knn.hip", r"constexpr int kLeaf = (\d+);"),
        max_k=find("atx_knn.hip", r"constexpr int kMaxK = (\d+);"),
        unroll=find("atx_superob.hip", r"constexpr int kSuperobUnroll = (\d+);"),
        long_group=find("atx_superob.hip", r"constexpr int64_t kLongGroup = (\d+);"),
        block=find("atx_common.hpp", r"constexpr int kBlock = (\d+);"),
        wave=find("atx_common.hpp", r"constexpr int kWave = (\d+);"),
        build_grid=find("atx_knn.hip", r"static unsigned blocks_for\(int64_t n\) \{[^}]*if \(b > (\d+)\) b = \1;"),
    )


K = read_constants()


@dataclass
class Kernels:
    """The callables under test.  ``knn_build(src, workspace=None)`` returns an index with ``n_src`` and
    ``query(tgt, k, out=None) -> (idx, d2)`` (``native.KnnIndex``); ``knn_workspace_bytes(n_src)``; ``cutout_inside(global_xyz,
    lam_xyz, neighbours, out=None)``; ``group_mean(values, order, offsets, mean, count)``; ``group_argmin(distance, order, offsets,
    nearest)`` — the signatures of ``native``."""

    knn_build: Callable
    knn_workspace_bytes: Callable
    cutout_inside: Callable
    group_mean: Callable
    group_argmin: Callable


def bits(a: np.ndarray) -> np.ndarray:
    """float64 bit patterns with every NaN made the same one (module docstring)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = a.view(np.int64).copy()
    out[np.isnan(a)] = np.int64(0x7FF8000000000000)
    return out


def to_dev(a: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class Guarded:
    """``data`` as a view inside a larger allocation: ``guard`` canary elements on either side."""

    def __init__(self, data: np.ndarray, device, canary, guard: int = 16):
        data = np.ascontiguousarray(data)
        flat = data.reshape(-1)
        self.host = np.concatenate([np.full(guard, canary, flat.dtype), flat, np.full(guard, canary, flat.dtype)])
        self.backing = torch.from_numpy(self.host.copy()).to(device)
        self.view = self.backing[guard: guard + flat.size].view(*data.shape) if data.ndim > 1 else self.backing[guard: guard + flat.size]
        self.guard, self.size = guard, flat.size

    def outside(self) -> np.ndarray:
        got = self.backing.cpu().numpy()
        return np.concatenate([got[: self.guard], got[self.guard + self.size:]]).view(np.uint8)

    def outside_before(self) -> np.ndarray:
        return np.concatenate([self.host[: self.guard], self.host[self.guard + self.size:]]).view(np.uint8)

    def canaries_intact(self) -> bool:
        return np.array_equal(self.outside(), self.outside_before())

    def unchanged(self) -> bool:
        return np.array_equal(self.backing.cpu().numpy().view(np.uint8), self.host.view(np.uint8))


# ================================================================================================================================
# k-NN
# ================================================================================================================================
def sq_distances(src: np.ndarray, x: np.ndarray) -> np.ndarray:
    """scipy's sqeuclidean_distance_double for 3-D points, one target against every source."""
    d = src - x
    s = np.zeros(len(src))
    s = s + d[:, 0] * d[:, 0]
    s = s + d[:, 1] * d[:, 1]
    s = s + d[:, 2] * d[:, 2]
    return s


def knn_reference(src: np.ndarray, tgt: np.ndarray, k: int):
    """``(idx int32 [n_tgt, k], d2 float64 [n_tgt, k])``: brute force, ``np.lexsort((index, s))``, padded with ``n_src`` / ``+inf``."""
    n_src = len(src)
    idx = np.full((len(tgt), k), n_src, dtype=np.int32)
    d2 = np.full((len(tgt), k), np.inf)
    for t, x in enumerate(tgt):
        s = sq_distances(src, x)
        if n_src > 4 * k:  # the candidates up to the k-th smallest distance, ties included; then the same lexsort
            cand = np.flatnonzero(s <= np.partition(s, k - 1)[k - 1])
        else:
            cand = np.arange(n_src)
        order = cand[np.lexsort((cand, s[cand]))][:k]
        idx[t, : len(order)] = order
        d2[t, : len(order)] = s[order]
    return idx, d2


def check_knn(kern: Kernels, device, name: str, src: np.ndarray, tgt: np.ndarray, ks, index=None) -> None:
    """Build (or take ``index``), query every k of ``ks``: every element of ``idx`` and ``d2`` of every row equals the brute force."""
    src, tgt = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(tgt, dtype=np.float64)
    if index is None:
        index = kern.knn_build(to_dev(src, device))
    t = to_dev(tgt, device)
    for k in ks:
        idx, d2 = index.query(t, k)
        got_i, got_d = idx.cpu().numpy(), d2.cpu().numpy()
        want_i, want_d = knn_reference(src, tgt, k)
        label = f"k-NN: {name}: n_src = {len(src)}, n_tgt = {len(tgt)}, k = {k}"
        assert got_i.dtype == np.int32 and got_i.shape == want_i.shape and got_d.shape == want_d.shape, f"{label}: shapes {got_i.shape}, {got_d.shape}"
        bad = np.argwhere(got_i != want_i)
        assert bad.size == 0, (f"{label}: {len(bad)} indices differ from the brute force, first at row {bad[0][0]}: kernel {got_i[bad[0][0]].tolist()}, "
                               f"lexsort {want_i[bad[0][0]].tolist()}, distances {want_d[bad[0][0]].tolist()}")
        bad = np.argwhere(bits(got_d) != bits(want_d))
        assert bad.size == 0, (f"{label}: {len(bad)} squared distances differ in bits, first at row {bad[0][0]}: kernel {got_d[bad[0][0]].tolist()}, "
                               f"brute force {want_d[bad[0][0]].tolist()}")


def sphere_points(rng, n: int) -> np.ndarray:
    """Unit vectors from latitudes and longitudes, as the host computes them (numpy deg2rad / cos / sin)."""
    lat, lon = np.deg2rad(rng.uniform(-90, 90, n)), np.deg2rad(rng.uniform(0, 360, n))
    return np.column_stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])


def latlon_xyz(lat, lon) -> np.ndarray:
    lat, lon = np.deg2rad(np.asarray(lat, dtype=np.float64)), np.deg2rad(np.asarray(lon, dtype=np.float64))
    return np.column_stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])


def knn_every_k(k: Constants = K) -> range:
    return range(1, k.max_k + 1)


def check_knn_every_k(kern: Kernels, device, ks=None, k: Constants = K) -> None:
    """Every template instance, 500 sources, 257 targets (one workgroup and one lane)."""
    rng = np.random.default_rng(500)
    src, tgt = sphere_points(rng, 500), sphere_points(rng, 257)
    tgt[:40] = src[rng.choice(500, 40, replace=False)]  # some targets on sources: d^2 = +0.0 first
    index = kern.knn_build(to_dev(src, device))
    check_knn(kern, device, "every neighbour count", src, tgt, list(knn_every_k(k)) if ks is None else ks, index=index)


def knn_source_sizes(k: Constants = K) -> list:
    """Around the leaf, the padded tree (leaf counts on both sides of a power of two) and a wave."""
    sizes = {1, 2, k.leaf - 1, k.leaf, k.leaf + 1, 2 * k.leaf - 1, 2 * k.leaf + 1, k.wave - 1, k.wave, k.wave + 1}
    for m in (3, 6):
        sizes |= {k.leaf * 2**m - 1, k.leaf * 2**m + 1}
    return sorted(s for s in sizes if s >= 1)


def knn_size_ks(n_src: int, k: Constants = K) -> list:
    """k below, at and above n_src where the instances reach (so that the padding is asked for), and the largest."""
    return sorted({1, 3, min(n_src, k.max_k), min(n_src + 1, k.max_k), k.max_k})


def check_knn_source_size(kern: Kernels, device, n_src: int, k: Constants = K) -> None:
    rng = np.random.default_rng(1000 + n_src)
    src, tgt = sphere_points(rng, n_src), sphere_points(rng, 65)
    tgt[0] = src[-1]  # the last point of the last (partial) leaf, at distance +0.0
    tgt[1] = src[0]
    check_knn(kern, device, "source sizes", src, tgt, knn_size_ks(n_src, k))


def knn_target_counts(k: Constants = K) -> list:
    return [1, k.wave - 1, k.wave, k.wave + 1, k.block - 1, k.block, k.block + 1]


def check_knn_target_count(kern: Kernels, device, n_tgt: int) -> None:
    rng = np.random.default_rng(2000 + n_tgt)
    src, tgt = sphere_points(rng, 300), sphere_points(rng, n_tgt)
    check_knn(kern, device, "target counts", src, tgt, (1, 4, 6))


def tie_sets() -> dict:
    """name -> (sources, targets, ks): point sets chosen so that distances tie exactly."""
    rng = np.random.default_rng(77)
    out = {}
    one = sphere_points(rng, 1)
    out["100 coincident sources"] = (np.repeat(one, 100, axis=0), np.vstack([one, sphere_points(rng, 6)]), (1, 3, 8, 9, 17))
    base = sphere_points(rng, 40)
    dup = np.repeat(base, 5, axis=0)[rng.permutation(200)]
    out["40 points, each five times, shuffled"] = (dup, np.vstack([base, sphere_points(rng, 25)]), (1, 2, 4, 5, 6, 10, 11))
    lat, lon = np.meshgrid(np.arange(-90.0, 91.0, 10.0), np.arange(0.0, 360.0, 10.0), indexing="ij")
    lattice = latlon_xyz(lat.ravel(), lon.ravel())
    clat, clon = np.meshgrid(np.arange(-85.0, 86.0, 10.0), np.arange(5.0, 360.0, 10.0), indexing="ij")
    centres = latlon_xyz(clat.ravel(), clon.ravel())
    pick = rng.choice(len(centres), 120, replace=False)
    out["10-degree lattice, its own points as targets"] = (lattice, lattice[:: 3], (1, 4, 5, 9))
    out["10-degree lattice, cell centres as targets"] = (lattice, centres[pick], (1, 4, 6, 16))
    # one great circle (the equator) at angles whose coordinates repeat under sign changes and a swap: eight sources at exactly the
    # same distance from either pole for every pair (a, b), in shuffled index order, far apart in Morton order
    ang = np.deg2rad(rng.uniform(1, 44, 16))
    a, b = np.cos(ang), np.sin(ang)
    ring = np.vstack([np.column_stack([sa * p, sb * q, np.zeros(16)]) for p, q in ((a, b), (b, a)) for sa in (1, -1) for sb in (1, -1)])
    ring = ring[rng.permutation(len(ring))]
    poles = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.5]])
    out["sources on one great circle"] = (ring, np.vstack([poles, ring[:20]]), (1, 2, 3, 7, 8, 9, 12, 17))
    pts = sphere_points(rng, 150)
    out["targets equal to sources"] = (pts, pts.copy(), (1, 2, 13))
    neg = sphere_points(rng, 90)
    neg[::3, 0], neg[1::3, 1], neg[2::3, 2] = -0.0, -0.0, -0.0
    tneg = neg[:30].copy()
    tneg[tneg == 0.0] = 0.0  # +0.0 in the target where the source has -0.0
    out["coordinates holding -0.0"] = (neg, np.vstack([tneg, sphere_points(rng, 10)]), (1, 3, 14))
    big = sphere_points(rng, 200) * 3.0
    out["points scaled by 3, off the unit sphere"] = (big, np.vstack([big[:20], sphere_points(rng, 40) * 3.0, sphere_points(rng, 10)]), (1, 4, 15))
    return out


def check_knn_ties(kern: Kernels, device, name: str) -> None:
    src, tgt, ks = tie_sets()[name]
    if name == "targets equal to sources":
        assert np.all(knn_reference(src, tgt, 1)[1].view(np.int64) == 0), "d^2 to the point itself is +0.0 bit for bit"
    check_knn(kern, device, f"ties: {name}", src, tgt, ks)


def aligned_workspace(n_bytes: int, device, canary: int = 0xC3, room: Optional[int] = None):
    """(backing, view): ``room or n_bytes`` bytes from a 256-byte boundary inside an allocation of canary bytes."""
    room = n_bytes if room is None else room
    backing = torch.full((room + 512 + 256,), canary, dtype=torch.uint8, device=device)
    shift = 256 + (-backing.data_ptr()) % 256
    return backing, backing[shift: shift + room], shift


def check_knn_reuse(kern: Kernels, device) -> None:
    """An index of 65 points built into the workspace that last held one of 3001; the same index queried twice."""
    rng = np.random.default_rng(3001)
    big, small, tgt = sphere_points(rng, 3001), sphere_points(rng, 65), sphere_points(rng, 130)
    n_big, n_small = kern.knn_workspace_bytes(3001), kern.knn_workspace_bytes(65)
    assert n_big >= n_small > 0
    _, ws, _ = aligned_workspace(n_big, device)
    first = kern.knn_build(to_dev(big, device), ws)
    check_knn(kern, device, "reuse: the 3001-point index", big, tgt, (4,), index=first)
    second = kern.knn_build(to_dev(small, device), ws)
    check_knn(kern, device, "reuse: 65 points in the workspace of 3001", small, tgt, (1, 4, 9), index=second)
    t = to_dev(tgt, device)
    a_i, a_d = second.query(t, 5)
    b_i, b_d = second.query(t, 5)
    assert np.array_equal(a_i.cpu().numpy(), b_i.cpu().numpy()) and np.array_equal(a_d.cpu().numpy().view(np.int64), b_d.cpu().numpy().view(np.int64)), \
        "k-NN: reuse: two queries of the same index differ"


def check_knn_buffers(kern: Kernels, device, n_src: int = 203, n_tgt: int = 67, k: int = 5) -> None:
    """Sources, targets and both outputs are views between canaries; the workspace ends in canary bytes."""
    rng = np.random.default_rng(n_src)
    src_h, tgt_h = sphere_points(rng, n_src), sphere_points(rng, n_tgt)
    src, tgt = Guarded(src_h, device, 0.123456789, guard=6), Guarded(tgt_h, device, -0.987654321, guard=6)
    idx = Guarded(np.full((n_tgt, k), -77, np.int32), device, -77)
    d2 = Guarded(np.full((n_tgt, k), -5.5), device, -5.5)
    n_bytes = kern.knn_workspace_bytes(n_src)
    backing, ws, shift = aligned_workspace(n_bytes, device)
    label = f"k-NN: buffers: n_src = {n_src}, n_tgt = {n_tgt}, k = {k}"

    def workspace_canaries():
        got = backing.cpu().numpy()
        return np.all(got[:shift] == 0xC3) and np.all(got[shift + n_bytes:] == 0xC3)

    index = kern.knn_build(src.view, ws)
    assert workspace_canaries(), f"{label}: the build wrote outside its {n_bytes} workspace bytes"
    assert src.unchanged(), f"{label}: the build modified the sources or their surroundings"
    got_i, got_d = index.query(tgt.view, k, out=(idx.view, d2.view))
    assert got_i.data_ptr() == idx.view.data_ptr() and got_d.data_ptr() == d2.view.data_ptr(), f"{label}: the query did not write into the given outputs"
    assert workspace_canaries(), f"{label}: the query wrote outside the workspace"
    assert src.unchanged() and tgt.unchanged(), f"{label}: the query modified sources or targets"
    assert idx.canaries_intact() and d2.canaries_intact(), f"{label}: written outside idx or d2"
    want_i, want_d = knn_reference(src_h, tgt_h, k)
    assert np.array_equal(idx.view.cpu().numpy(), want_i), f"{label}: indices differ from the brute force"
    assert np.array_equal(bits(d2.view.cpu().numpy()), bits(want_d)), f"{label}: squared distances differ in bits"


def check_knn_past_the_cap(kern: Kernels, device, k: Constants = K) -> dict:
    """More padded leaves than four sweeps of the capped leaf loop, a first merge level of two sweeps; two targets, k = 4."""
    n_src = k.past_cap_sources()
    leaves = -(-n_src // k.leaf)
    n_pow2 = 1 << (leaves - 1).bit_length()
    assert n_pow2 == 4 * k.build_sweep and n_pow2 // 2 == 2 * k.build_sweep and leaves > n_pow2 // 2 and n_src % k.leaf == 1
    rng = np.random.default_rng(n_src)
    z, lon = rng.uniform(-1, 1, n_src), rng.uniform(0, 2 * np.pi, n_src)
    r = np.sqrt(1 - z * z)
    src = np.column_stack([r * np.cos(lon), r * np.sin(lon), z])
    del z, lon, r
    tgt = np.vstack([src[n_src - 3], sphere_points(rng, 1)])
    check_knn(kern, device, "past the cap", src, tgt, (4,))
    return {"n_src": n_src, "leaves": leaves, "padded leaves": n_pow2, "sweep": k.build_sweep, "workspace bytes": kern.knn_workspace_bytes(n_src)}


# ================================================================================================================================
# cutout
# ================================================================================================================================
EPSILON = 0.0000001


def fma(a: float, b: float, c: float) -> float:
    """round(a * b + c), one rounding."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def dot3(a, b) -> float:
    return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0]))


def cross3(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def ray_triangle(d, v0, v1, v2) -> dict:
    """Möller–Trumbore from the origin along ``d``, as the kernel states it: ``{"a", "u", "v", "uv", "t", "hit"}`` (what was reached)."""
    d, v0, v1, v2 = ([float(x) for x in p] for p in (d, v0, v1, v2))
    e1 = [v1[c] - v0[c] for c in range(3)]
    e2 = [v2[c] - v0[c] for c in range(3)]
    s = [0.0 - v0[c] for c in range(3)]
    h = cross3(d, e2)
    out = {"a": dot3(e1, h), "hit": False}
    if -EPSILON < out["a"] < EPSILON:
        return out
    f = 1.0 / out["a"]
    u = out["u"] = f * dot3(s, h)
    if u < 0.0 or u > 1.0:
        return out
    q = cross3(s, e1)
    v = out["v"] = f * dot3(d, q)
    out["uv"] = u + v
    if v < 0.0 or u + v > 1.0:
        return out
    out["t"] = f * dot3(e2, q)
    out["hit"] = out["t"] > EPSILON
    return out


def cutout_reference(g: np.ndarray, lam: np.ndarray, nb: np.ndarray) -> np.ndarray:
    """uint8 [n]: a triangle with an index outside [0, n_lam) is skipped."""
    n, k = nb.shape
    n_lam = len(lam)
    inside = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        for j in range(k):
            tri = (int(nb[i, j]), int(nb[i, (j + 1) % k]), int(nb[i, (j + 2) % k]))
            if any(t < 0 or t >= n_lam for t in tri):
                continue
            if ray_triangle(g[i], lam[tri[0]], lam[tri[1]], lam[tri[2]])["hit"]:
                inside[i] = 1
                break
    return inside


SENTINEL_POINT = (0.25, -0.5, 0.75)  # finite: a lost index guard reads it and computes a wrong bit, inside the allocation


def run_cutout(kern: Kernels, device, name: str, g: np.ndarray, lam: np.ndarray, nb: np.ndarray, want: Optional[np.ndarray] = None) -> np.ndarray:
    """``lam`` between sentinel rows, ``inside`` between canaries; every byte equals the reference; the inputs are unchanged."""
    g, lam, nb = np.ascontiguousarray(g, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(lam, dtype=np.float64), np.ascontiguousarray(nb, dtype=np.int32)
    n, k = nb.shape
    assert len(g) == n
    lam_host = np.vstack([np.tile(SENTINEL_POINT, (3, 1)), lam, np.tile(SENTINEL_POINT, (3, 1))])
    lam_back = to_dev(lam_host, device)
    gd = to_dev(g, device) if n else torch.zeros((0, 3), dtype=torch.float64, device=device)
    nbd = to_dev(nb, device) if n else torch.zeros((0, k), dtype=torch.int32, device=device)
    out = Guarded(np.full(n, 0x5A, np.uint8), device, 0x5A)
    kern.cutout_inside(gd, lam_back[3: 3 + len(lam)], nbd, out=out.view)
    got = out.view.cpu().numpy()
    want = cutout_reference(g, lam, nb) if want is None else want
    label = f"cutout: {name}: n = {n}, k = {k}, n_lam = {len(lam)}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{label}: {bad.size} points differ from the reference, first at {bad[:5].tolist()}: kernel {got[bad[:5]].tolist()}, reference {want[bad[:5]].tolist()}"
    assert out.canaries_intact(), f"{label}: written outside inside[0:n)"
    assert np.array_equal(lam_back.cpu().numpy().view(np.int64), lam_host.view(np.int64)), f"{label}: lam_xyz was modified"
    if n:
        assert np.array_equal(gd.cpu().numpy().view(np.int64), g.view(np.int64)) and np.array_equal(nbd.cpu().numpy(), nb), f"{label}: an input was modified"
    return got


def lam_patch(seed: int = 5):
    """A jittered 12 x 12 limited-area patch around 45N 5E."""
    rng = np.random.default_rng(seed)
    lat, lon = np.meshgrid(40.0 + np.arange(12.0), np.arange(12.0), indexing="ij")
    lat, lon = lat + rng.uniform(-0.3, 0.3, lat.shape), lon + rng.uniform(-0.3, 0.3, lon.shape)
    return latlon_xyz(lat.ravel(), lon.ravel())


def patch_points(seed: int, n: int) -> np.ndarray:
    """Points over the patch and a margin around it (some are outside)."""
    rng = np.random.default_rng(seed)
    return latlon_xyz(rng.uniform(38.0, 53.0, n), rng.uniform(-2.0, 13.0, n))


# (k, n): every k of the issue, every n; a few thousand point-triangle pairs in all (20 000 rational fmas take 0.3 s)
CUTOUT_SHAPES = ((1, 1), (1, 65), (2, 65), (3, 0), (3, 1), (3, 255), (3, 256), (3, 257), (4, 257), (5, 65), (17, 65))


def check_cutout_patch(kern: Kernels, device, k: int, n: int, c: Constants = K) -> None:
    assert k <= c.max_k
    lam = lam_patch()
    g = patch_points(100 * k + n, n)
    nb = knn_reference(lam, g, k)[0] if n else np.zeros((0, k), np.int32)
    got = run_cutout(kern, device, "neighbour tables of a jittered patch", g, lam, nb)
    if k >= 3 and n >= 65:
        assert 0 < got.sum() < n, "cutout: the patch case has points inside and points outside"
    if k <= 2:
        assert got.sum() == 0, "cutout: a table of one or two neighbours has only degenerate triangles"


def check_cutout_edge_points(kern: Kernels, device) -> None:
    """Points that lie on the edges and vertices of a REGULAR patch's triangles as far as float64 can say (midpoints and thirds of
    neighbouring grid points, the grid points themselves): u, v and u + v come out within a rounding of 0 and 1, so the answer is
    the arithmetic's — one rounding per dot term or two."""
    lat, lon = np.meshgrid(40.0 + np.arange(8.0), np.arange(8.0), indexing="ij")
    lam = latlon_xyz(lat.ravel(), lon.ravel())
    pts = []
    for i in range(1, 7):
        for j in range(1, 7, 2):
            c = lam[i * 8 + j]
            for other in (lam[i * 8 + j + 1], lam[(i + 1) * 8 + j], lam[(i + 1) * 8 + j + 1], lam[(i - 1) * 8 + j - 1]):
                pts += [(c + other) * 0.5, (c + other + other) / 3.0]
            pts.append(c)
    g = np.array(pts)
    nb = knn_reference(lam, g, 4)[0]
    run_cutout(kern, device, "points on the edges of a regular patch", g, lam, nb)


def exact_triangles():
    """(name, v0, v1, v2): small-integer vertices scaled by a power of two; ``a`` is a power of two of either sign, so f, u, v are exact."""
    out = []
    for scale in (0.5, 0.125):
        v = np.array([[2.0, -1.0, -1.0], [2.0, 1.0, -1.0], [2.0, -1.0, 1.0]]) * scale
        out.append((f"x-facing, a < 0, scale {scale}", v[0], v[1], v[2]))
        out.append((f"x-facing, a > 0, scale {scale}", v[0], v[2], v[1]))
        w = v[:, [2, 0, 1]]
        out.append((f"y-facing, scale {scale}", w[0], w[1], w[2]))
    return out


def check_cutout_constructed(kern: Kernels, device) -> None:
    """Points exactly on a vertex and on an edge: the reference's u, v, u + v are exactly 0 or 1 there and it takes the boundary as
    INSIDE (it rejects ``u < 0``, ``u > 1``, ``v < 0``, ``u + v > 1``: the closed triangle); one float outside the edge is outside."""
    for name, v0, v1, v2 in exact_triangles():
        lam = np.vstack([v0, v1, v2, v0 + (v1 - v0) * 8 + (v2 - v0) * 8])  # a fourth point far away, never in a row
        pts, states = [], []
        for what, p, exact in (("vertex 0", v0, {"u": 0.0, "v": 0.0}), ("vertex 1", v1, {"u": 1.0, "v": 0.0, "uv": 1.0}), ("vertex 2", v2, {"u": 0.0, "v": 1.0, "uv": 1.0}),
                               ("edge 0-1", (v0 + v1) / 2, {"v": 0.0}), ("edge 0-2", (v0 + v2) / 2, {"u": 0.0}), ("edge 1-2", (v1 + v2) / 2, {"uv": 1.0}),
                               ("centre", (v0 + v1 + v2) / 4 + v0 / 4, {})):
            r = ray_triangle(p, v0, v1, v2)
            assert r["hit"] and r["t"] == 1.0 and all(r[key] == val for key, val in exact.items()), f"cutout: {name}: {what}: the reference gives {r}"
            pts.append(p)
            states.append(1)
        # one float beyond edge 0-1 (v < 0) and beyond edge 0-2 (u < 0), and twice the point of edge 1-2 mirrored out (u + v > 1)
        e1, e2 = v1 - v0, v2 - v0
        for what, p in (("beyond edge 0-1", (v0 + v1) / 2 - e2 * 2.0**-40), ("beyond edge 0-2", (v0 + v2) / 2 - e1 * 2.0**-40),
                        ("beyond edge 1-2", (v1 + v2) / 2 + (e1 + e2) * 2.0**-40)):
            assert not any(ray_triangle(p, *tri)["hit"] for tri in ((v0, v1, v2), (v1, v2, v0), (v2, v0, v1))), f"cutout: {name}: {what} is outside"
            pts.append(p)
            states.append(0)
        g = np.array(pts)
        nb = np.tile(np.array([0, 1, 2], np.int32), (len(g), 1))
        assert np.array_equal(cutout_reference(g, lam, nb), np.array(states, np.uint8))
        run_cutout(kern, device, f"constructed: {name}", g, lam, nb, want=np.array(states, np.uint8))
        # one rotation alone: the "not found" marker in a row of four leaves only the triangle (row[0], row[1], row[2]), so each
        # rotation has to take its own boundary (with all three a point rejected by one rotation is accepted by another)
        for rot in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            nb4 = np.tile(np.array([*rot, len(lam)], np.int32), (len(g), 1))
            tri = [lam[r] for r in rot]
            assert [int(ray_triangle(p, *tri)["hit"]) for p in g] == states
            run_cutout(kern, device, f"constructed: {name}: rotation {rot} alone", g, lam, nb4, want=np.array(states, np.uint8))


def epsilon_triangles():
    """(name, d, v0, v1, v2, a, inside): triangles whose ``a`` is the double just inside and just outside ±1e-7.
    Constructed: d = (0,0,1), e2 = (0,-1,0) give h = (1,0,0) and a = e1[0] exactly.  Searched: a generic triangle's second vertex
    moved along its edge by bisection on the reference until two ADJACENT doubles of the step give |a| < 1e-7 and |a| >= 1e-7."""
    out = []
    d = np.array([0.0, 0.0, 1.0])
    for sign in (1.0, -1.0):
        for x, what in ((EPSILON, "at"), (math.nextafter(EPSILON, 0.0), "just inside"), (math.nextafter(EPSILON, 1.0), "just outside")):
            v0, v1, v2 = np.array([0.0, 0.0, 1.0]), np.array([sign * x, 0.0, 1.0]), np.array([0.0, -1.0, 1.0])
            r = ray_triangle(d, v0, v1, v2)
            assert r["a"] == sign * x and r["hit"] == (what != "just inside"), r
            out.append((f"a {what} {sign * EPSILON!r} (constructed)", d, v0, v1, v2, r["a"], r["hit"]))
    for sign in (1.0, -1.0):
        v0 = latlon_xyz([45.0], [5.0])[0]
        v2 = latlon_xyz([45.8], [5.1])[0]
        direction = (latlon_xyz([45.1], [5.9])[0] - v0) * sign
        dd = v0 + (v2 - v0) * 1e-3 + direction * 1e-12  # a ray through the sliver next to its edge 0-2
        lo, hi = 0.0, 1.0
        assert abs(ray_triangle(dd, v0, v0 + direction * hi, v2)["a"]) >= EPSILON
        while math.nextafter(lo, hi) < hi:
            mid = lo + (hi - lo) / 2
            if abs(ray_triangle(dd, v0, v0 + direction * mid, v2)["a"]) < EPSILON:
                lo = mid
            else:
                hi = mid
        for step, what in ((lo, "just inside"), (hi, "just outside")):
            v1 = v0 + direction * step
            r = ray_triangle(dd, v0, v1, v2)
            assert (abs(r["a"]) < EPSILON) == (what == "just inside")
            out.append((f"a = {r['a']!r} {what} (searched)", dd, v0, v1, v2, r["a"], r["hit"]))
    return out


def check_cutout_epsilon(kern: Kernels, device) -> None:
    cases = epsilon_triangles()
    assert {c[6] for c in cases} == {True, False}
    for name, d, v0, v1, v2, _, _ in cases:
        lam = np.vstack([v0, v1, v2])
        # k = 3 asks all three rotations; rotations of a sliver may differ in a, so the reference decides the row
        nb = np.array([[0, 1, 2]], np.int32)
        run_cutout(kern, device, f"epsilon: {name}", d.reshape(1, 3), lam, nb)


def check_cutout_stray(kern: Kernels, device) -> None:
    """-1 and n_lam in neighbour rows: the row equals the reference with those triangles skipped."""
    lam = lam_patch()
    n_lam = len(lam)
    g = patch_points(999, 96)
    rng = np.random.default_rng(999)
    for k in (3, 5):
        nb = knn_reference(lam, g, k)[0].copy()
        clean = cutout_reference(g, lam, nb)
        assert clean.sum() >= 16  # rows that are inside: a stray index takes triangles away from them
        for r in range(len(g)):
            if r % 3 == 0:
                nb[r, rng.integers(0, k)] = -1 if r % 2 else n_lam
            elif r % 7 == 0:
                nb[r, :] = rng.choice(np.array([-1, n_lam], np.int32), k)
        want = cutout_reference(g, lam, nb)
        assert np.any(want != clean), "cutout: stray indices change at least one row of the reference"
        run_cutout(kern, device, "stray indices -1 and n_lam", g, lam, nb, want=want)


# ================================================================================================================================
# superob
# ================================================================================================================================
SENTINEL_VALUE = 12345.678  # finite: what a lost row guard would read, inside the test's own allocation
MEAN_CANARY, COUNT_CANARY, NEAREST_CANARY = -6.02e23, -4242, -99


class Table:
    """A table of ``n_obs`` rows of which ``sum(lengths)`` are selected, in groups of the given lengths; ``order`` is the stable group
    order of the (shuffled) rows.  ``values`` [n_cols, n_obs] host float64; ``put(c, g, k, v)`` sets the k-th row of group g."""

    def __init__(self, lengths, n_cols: int, seed: int, unselected: int = 0, shuffle: bool = True, nan_share: float = 0.1):
        rng = np.random.default_rng(seed)
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.n_groups, self.n_sel = len(self.lengths), int(self.lengths.sum())
        self.n_obs = self.n_sel + unselected
        labels = np.full(self.n_obs, -1, dtype=np.int64)
        rows = rng.permutation(self.n_obs)[: self.n_sel] if shuffle else np.arange(self.n_sel)
        per_row = np.repeat(np.arange(self.n_groups), self.lengths)
        labels[rows] = rng.permutation(per_row) if shuffle else per_row
        sel = np.flatnonzero(labels >= 0)
        self.order = sel[np.argsort(labels[sel], kind="stable")].astype(np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.values = rng.standard_normal((n_cols, self.n_obs)) * 10.0 ** rng.integers(-8, 9, (n_cols, self.n_obs))
        self.values[rng.random((n_cols, self.n_obs)) < nan_share] = np.nan
        self.n_cols = n_cols

    def put(self, c: int, g: int, k: int, v: float) -> None:
        assert 0 <= k < self.lengths[g]
        self.values[c, self.order[self.offsets[g] + k]] = v

    def fill(self, c: int, g: int, v: float) -> None:
        self.values[c, self.order[self.offsets[g]: self.offsets[g + 1]]] = v


def segment_rows(order: np.ndarray, offsets: np.ndarray, g: int, n_sel: int):
    """The row indices of group g, or None for a bad segment."""
    b, e = int(offsets[g]), int(offsets[g + 1])
    if b < 0 or e < b or e > n_sel:
        return None
    return order[b:e].astype(np.int64)


def column_values(col: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """The column at ``rows``; a row index outside the column takes no part (NaN)."""
    ok = (rows >= 0) & (rows < len(col))
    out = np.full(len(rows), np.nan)
    out[ok] = col[rows[ok]]
    return out


def mean_reference(values: np.ndarray, order: np.ndarray, offsets: np.ndarray):
    """``(mean [n_cols, n_groups], count [n_cols, n_groups])`` by the scalar Kahan loop; a bad segment gives NaN and 0."""
    n_cols, n_groups, n_sel = values.shape[0], len(offsets) - 1, len(order)
    mean, count = np.full((n_cols, n_groups), np.nan), np.zeros((n_cols, n_groups), dtype=np.int64)
    for c in range(n_cols):
        groups, which = [], []
        for g in range(n_groups):
            rows = segment_rows(order, offsets, g, n_sel)
            if rows is not None:
                groups.append(column_values(values[c], rows))
                which.append(g)
        if groups:
            mean[c, which] = kahan_means_of_many(groups)
            count[c, which] = [int((~np.isnan(v)).sum()) for v in groups]
            for j in sorted({0, len(groups) // 2, len(groups) - 1}):  # the vectorised loop against the scalar one
                m, n = kahan_mean(groups[j])
                assert bits(np.array([m]))[0] == bits(mean[c, which[j]: which[j] + 1])[0] and n == count[c, which[j]]
    return mean, count


def argmin_reference(distance: np.ndarray, order: np.ndarray, offsets: np.ndarray) -> np.ndarray:
    """int32 [n_groups]: strict ``<`` in row order, the first non-NaN taken even when +inf, all NaN: the first row; -1 for a bad
    segment, an empty group, or a first row that is no row."""
    n_groups, n_sel, n_obs = len(offsets) - 1, len(order), len(distance)
    out = np.full(n_groups, -1, dtype=np.int32)
    for g in range(n_groups):
        rows = segment_rows(order, offsets, g, n_sel)
        if rows is None or len(rows) == 0:
            continue
        best, best_d, found = int(rows[0]), INF, False
        for r, v in zip(rows.tolist(), column_values(distance, rows).tolist()):
            if v < best_d or (not found and v == v):
                best, best_d, found = r, v, True
        out[g] = best if 0 <= best < n_obs else -1
    return out


def run_group_mean(kern: Kernels, device, name: str, values: np.ndarray, order: np.ndarray, offsets: np.ndarray, val_slack: int = 0, out_slack: int = 0,
                   want=None):
    """Every input a view between finite sentinels (two elements at least), ``values`` pitched by ``n_obs + val_slack``, the outputs
    pitched by ``n_groups + out_slack`` between canaries.  Every mean (bits) and count equals the reference."""
    n_cols, n_obs = values.shape
    n_groups, n_sel = len(offsets) - 1, len(order)
    pitch = n_obs + val_slack
    vhost = np.full((n_cols, pitch), SENTINEL_VALUE)
    vhost[:, :n_obs] = values
    vals = Guarded(vhost, device, SENTINEL_VALUE, guard=4)
    ords = Guarded(np.concatenate([order, np.zeros(4, np.int32)]).astype(np.int32), device, 0, guard=4)  # slack after n_sel: row 0
    offs = Guarded(offsets.astype(np.int64), device, 0, guard=4)
    opitch = n_groups + out_slack
    mean = Guarded(np.full((n_cols, opitch), MEAN_CANARY), device, MEAN_CANARY)
    count = Guarded(np.full((n_cols, opitch), COUNT_CANARY, np.int64), device, COUNT_CANARY)
    kern.group_mean(vals.view[:, :n_obs], ords.view[:n_sel], offs.view, mean.view[:, :n_groups], count.view[:, :n_groups])
    got_m, got_c = mean.view.cpu().numpy(), count.view.cpu().numpy()
    want_m, want_c = want if want is not None else mean_reference(values, order, offsets)
    label = f"group mean: {name}: {n_groups} groups, {n_cols} columns, n_obs = {n_obs}, n_sel = {n_sel}, val_pitch = {pitch}, out_pitch = {opitch}"
    bad = np.argwhere(bits(got_m[:, :n_groups]) != bits(want_m))
    lens = np.diff(offsets)
    assert bad.size == 0, (f"{label}: {len(bad)} means differ in bits from the Kahan loop, first (column, group) {bad[:4].tolist()} of lengths {lens[bad[:4, 1]].tolist()}: "
                           f"kernel {[got_m[c, g] for c, g in bad[:4]]}, reference {[want_m[c, g] for c, g in bad[:4]]}")
    bad = np.argwhere(got_c[:, :n_groups] != want_c)
    assert bad.size == 0, f"{label}: {len(bad)} counts differ, first (column, group) {bad[:4].tolist()}: kernel {[got_c[c, g] for c, g in bad[:4]]}, reference {[want_c[c, g] for c, g in bad[:4]]}"
    assert np.all(got_m[:, n_groups:] == MEAN_CANARY) and np.all(got_c[:, n_groups:] == COUNT_CANARY), f"{label}: written into the slack of the output pitch"
    assert mean.canaries_intact() and count.canaries_intact(), f"{label}: written outside mean or count"
    assert vals.unchanged() and ords.unchanged() and offs.unchanged(), f"{label}: an input was modified"
    return got_m[:, :n_groups], got_c[:, :n_groups]


def run_group_argmin(kern: Kernels, device, name: str, distance: np.ndarray, order: np.ndarray, offsets: np.ndarray, want=None):
    n_obs, n_groups, n_sel = len(distance), len(offsets) - 1, len(order)
    dist = Guarded(distance, device, SENTINEL_VALUE * -1.0, guard=4)  # a lost guard would find a NEGATIVE sentinel the smallest
    ords = Guarded(np.concatenate([order, np.zeros(4, np.int32)]).astype(np.int32), device, 0, guard=4)
    offs = Guarded(offsets.astype(np.int64), device, 0, guard=4)
    near = Guarded(np.full(n_groups, NEAREST_CANARY, np.int32), device, NEAREST_CANARY)
    kern.group_argmin(dist.view, ords.view[:n_sel], offs.view, near.view)
    got = near.view.cpu().numpy()
    want = argmin_reference(distance, order, offsets) if want is None else want
    label = f"group argmin: {name}: {n_groups} groups, n_obs = {n_obs}, n_sel = {n_sel}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{label}: {bad.size} groups differ from the row-order loop, first {bad[:5].tolist()} of lengths {np.diff(offsets)[bad[:5]].tolist()}: kernel {got[bad[:5]].tolist()}, reference {want[bad[:5]].tolist()}"
    assert near.canaries_intact(), f"{label}: written outside nearest"
    assert dist.unchanged() and ords.unchanged() and offs.unchanged(), f"{label}: an input was modified"
    return got


def edge_lengths(k: Constants = K) -> list:
    """1, around the unroll and twice the unroll, around a wave, around kLongGroup, kLongGroup plus a wave, twice kLongGroup, 1000."""
    u, w, big = k.unroll, k.wave, k.long_group
    out = [1]
    for m in (u, 2 * u, w, big, big + w, 2 * big):
        out += [m - 1, m, m + 1]
    return out + [1000]


# --- order-dependence of the chosen values: what makes the long groups a test of the summation ORDER ---
def pairwise_sum(v: np.ndarray) -> float:
    return float(v[0]) if len(v) == 1 else pairwise_sum(v[: len(v) // 2]) + pairwise_sum(v[len(v) // 2:])


def lane_partials_mean(v: np.ndarray, wave: int) -> float:
    """Per-lane Kahan partials (lane j takes rows j, j + wave, ...) added up in lane order."""
    v = v[~np.isnan(v)]
    if len(v) == 0:
        return NAN
    total = 0.0
    for j in range(wave):
        part = comp = 0.0
        for x in v[j::wave].tolist():
            y = x - comp
            t = part + y
            comp = (t - part) - y
            part = t
        total += part
    return total / len(v)


def check_values_depend_on_order(values: np.ndarray, order: np.ndarray, offsets: np.ndarray, k: Constants = K) -> int:
    """Among the long groups, a pairwise sum and a per-lane-partials sum each differ from the sequential Kahan mean in at least one
    bit.  Returns the number of long groups looked at."""
    seen = pair = lanes = 0
    for g in range(len(offsets) - 1):
        if offsets[g + 1] - offsets[g] < k.long_group:
            continue
        v = values[0][order[offsets[g]: offsets[g + 1]]]
        v = v[~np.isnan(v)]
        if len(v) == 0 or not np.all(np.isfinite(v)):
            continue
        seq = kahan_mean(v)[0]
        seen += 1
        pair += pairwise_sum(v) / len(v) != seq
        lanes += lane_partials_mean(v, k.wave) != seq
    assert seen and pair and lanes, f"the values do not tell summation orders apart: {seen} long groups, pairwise differs in {pair}, lane partials in {lanes}"
    return seen


def check_mean_edge_lengths(kern: Kernels, device, shuffled: bool, k: Constants = K) -> None:
    """One launch whose groups have every edge length, in that order or shuffled; 5 columns, a selection of part of the table, pitched."""
    lengths = np.array(edge_lengths(k))
    if shuffled:
        lengths = lengths[np.random.default_rng(8).permutation(len(lengths))]
    t = Table(lengths, n_cols=5, seed=21 + shuffled, unselected=37)
    assert t.n_sel < t.n_obs
    assert check_values_depend_on_order(t.values, t.order, t.offsets, k) >= 9
    run_group_mean(kern, device, f"edge lengths {'shuffled' if shuffled else 'in order'}", t.values, t.order, t.offsets, val_slack=5, out_slack=3)
    d = t.values[1].copy()
    run_group_argmin(kern, device, f"edge lengths {'shuffled' if shuffled else 'in order'}", d, t.order, t.offsets)


def group_count_cases(k: Constants = K) -> dict:
    """name -> (lengths, n_cols): group counts around a wave, a workgroup and two; long groups at lanes 0, 1 and 63 of one wave, as
    the last group of a partial workgroup (beside lanes with g >= n_groups), and a table of long groups only."""
    w, b, big = k.wave, k.block, k.long_group
    rng = np.random.default_rng(64)
    out = {}
    for n in (1, w - 1, w, w + 1, b - 1, b, b + 1, 2 * b + 1):
        lengths = rng.integers(1, 13, n)
        where = [g for g in (0, 1, w - 1) if g < n and n >= w] + ([n - 1] if n % b in (1, w + 1) and n > 1 else [])
        for j, g in enumerate(where):
            lengths[g] = big + (0, 1, 44, w + 5)[j % 4]
        out[f"{n} groups, long at {where}"] = (lengths, 1 + (n % 2))
    out["1 long group"] = (np.array([big + 3]), 2)
    out[f"{w + 1} long groups only"] = (rng.integers(big, big + w + 10, w + 1), 1)
    return out


def check_mean_group_counts(kern: Kernels, device, name: str, k: Constants = K) -> None:
    lengths, n_cols = group_count_cases(k)[name]
    t = Table(lengths, n_cols=n_cols, seed=len(lengths), unselected=11)
    run_group_mean(kern, device, name, t.values, t.order, t.offsets, val_slack=2, out_slack=2 if n_cols > 1 else 0)
    run_group_argmin(kern, device, name, t.values[0], t.order, t.offsets)


def check_mean_special_values(kern: Kernels, device, k: Constants = K) -> None:
    """+inf then finite values, +inf then -inf (the compensation reset), an all-NaN group, -0.0 alone: each once in a short group and
    once from a position >= a wave of a long group."""
    big, w = k.long_group + 44, k.wave
    patterns = {"+inf then finite": [INF, 1.5, -2.25e-3, 7e5], "+inf then -inf": [INF, -INF, 3.0], "finite, +inf, finite": [1e-8, INF, 1e8, 1.0],
                "-inf then finite": [-INF, 1.0, 2.0], "-0.0 alone": [-0.0], "all NaN": [NAN]}
    lengths = []
    for _ in patterns:
        lengths += [5, big]
    lengths += [1, 3]
    t = Table(np.array(lengths), n_cols=2, seed=99, unselected=9)
    where = {}
    for j, (name, vals) in enumerate(patterns.items()):
        short, long_ = 2 * j, 2 * j + 1
        for c in range(2):
            if name in ("-0.0 alone", "all NaN"):
                t.fill(c, short, NAN)
                t.fill(c, long_, NAN)
            if name == "-0.0 alone":
                t.put(c, short, 2, -0.0)
                t.put(c, long_, w + 7, -0.0)
            elif name != "all NaN":
                for i, v in enumerate(vals):
                    t.put(c, short, i, v)
                    t.put(c, long_, w + 3 + i, v)
        where[name] = (short, long_)
    t.put(0, len(lengths) - 2, 0, -0.0)  # a group of one row
    want_m, want_c = mean_reference(t.values, t.order, t.offsets)
    s, l = where["all NaN"]
    assert want_c[0, s] == 0 and want_c[0, l] == 0 and np.isnan(want_m[0, [s, l]]).all()
    s, l = where["-0.0 alone"]
    assert want_c[0, s] == 1 and want_c[0, l] == 1 and np.array_equal(want_m[0, [s, l]].view(np.int64), np.zeros(2, np.int64)), "module docstring: +0.0"
    s, l = where["+inf then finite"]
    assert want_m[0, s] == INF and want_m[0, l] == INF
    s, l = where["+inf then -inf"]
    assert np.isnan(want_m[0, [s, l]]).all() and want_c[0, s] > 0
    run_group_mean(kern, device, "special values", t.values, t.order, t.offsets, val_slack=3, out_slack=4, want=(want_m, want_c))


def check_argmin_walk(kern: Kernels, device, length: int) -> None:
    """``length`` groups of ``length`` rows; group i has its unique minimum at position i."""
    t = Table(np.full(length, length), n_cols=1, seed=length, nan_share=0.0)
    d = np.random.default_rng(length).uniform(1.0, 2.0, t.n_obs)
    for g in range(length):
        d[t.order[t.offsets[g] + g]] = 0.5
    want = t.order[t.offsets[:-1] + np.arange(length)].astype(np.int32)
    assert np.array_equal(argmin_reference(d, t.order, t.offsets), want)
    run_group_argmin(kern, device, f"the minimum walked through a group of {length}", d, t.order, t.offsets, want=want)


def check_argmin_edge_groups(kern: Kernels, device, k: Constants = K) -> None:
    """Equal minima in different lanes, ±0.0 in both orders, +inf the only number, NaN first, all NaN — in short and in long groups."""
    w = k.wave
    big = k.long_group + w + 9
    cases = []  # (name, length, {position: value}, background, position expected)
    for length in (7, big):
        far = [3, w + 3, 2 * w + 2] if length == big else [3, 4, 6]
        cases += [
            ("equal minima", length, {p: 0.25 for p in far}, 1.0, far[0]),
            ("equal minima, the lowest position in a high lane", length, {far[2]: 0.25, w + 40: 0.25} if length == big else {5: 0.25, 6: 0.25}, 1.0,
             w + 40 if length == big else 5),
            ("+0.0 before -0.0", length, {far[0]: 0.0, far[1]: -0.0}, 1.0, far[0]),
            ("-0.0 before +0.0", length, {far[0]: -0.0, far[1]: 0.0}, 1.0, far[0]),
            ("+inf the only number", length, {far[1]: INF}, NAN, far[1]),
            ("+inf twice among NaN", length, {far[1]: INF, far[2]: INF}, NAN, far[1]),
            ("NaN first, then numbers", length, {0: NAN, 1: NAN, far[1]: 2.0, far[2]: 2.0}, 5.0, far[1]),
            ("all NaN", length, {}, NAN, 0),
            ("-inf twice", length, {far[1]: -INF, far[2]: -INF}, 1.0, far[1]),
        ]
    t = Table(np.array([c[1] for c in cases]), n_cols=1, seed=4, unselected=5)
    d = np.full(t.n_obs, 9.0)
    want = np.zeros(len(cases), np.int32)
    for g, (_, length, spots, background, at) in enumerate(cases):
        rows = t.order[t.offsets[g]: t.offsets[g + 1]]
        d[rows] = background
        for p, v in spots.items():
            d[rows[p]] = v
        want[g] = rows[at]
    ref = argmin_reference(d, t.order, t.offsets)
    assert np.array_equal(ref, want), f"argmin edge groups: the reference gives {ref.tolist()}, the case states {want.tolist()}"
    run_group_argmin(kern, device, "edge groups", d, t.order, t.offsets, want=want)


def check_superob_guards(kern: Kernels, device, k: Constants = K) -> None:
    """Bad segment bounds give NaN / count 0 / nearest -1 and bad row indices take no part; every neighbouring group is exact.  Every
    stray value stays within the two elements of finite sentinel slack that surround each input."""
    lengths = np.array([5, k.long_group + 70, 9, 1, k.long_group, 12, 3])
    base = Table(lengths, n_cols=2, seed=31, unselected=6, nan_share=0.05)
    n_groups, n_sel, n_obs = base.n_groups, base.n_sel, base.n_obs
    def offsets_with(at: int, value: int) -> np.ndarray:
        off = base.offsets.copy()
        off[at] = value
        return off

    # (name, order, offsets, the groups whose segment is bad)
    variants = [
        ("a negative start", base.order, offsets_with(0, -1), [0]),
        ("a start of -2", base.order, offsets_with(0, -2), [0]),
        ("end < begin", base.order, offsets_with(3, base.offsets[2] - 1), [2]),
        ("end < begin for a long group", base.order, offsets_with(2, base.offsets[1] - 1), [1]),
        ("end == n_sel + 1", base.order, offsets_with(n_groups, n_sel + 1), [n_groups - 1]),
    ]
    for stray in (-1, -2, n_obs, n_obs + 1):
        order = base.order.copy()
        for g, p in ((0, 2), (1, k.wave + 5), (1, 0), (3, 0), (4, k.long_group - 1)):
            order[base.offsets[g] + p] = stray
        variants.append((f"row index {stray}", order, base.offsets, []))
    for name, order, offsets, bad in variants:
        want_m, want_c = mean_reference(base.values, order, offsets)
        want_n = argmin_reference(base.values[0], order, offsets)
        for g in bad:
            assert np.isnan(want_m[:, g]).all() and np.all(want_c[:, g] == 0) and want_n[g] == -1
        if name.startswith("row index"):
            assert want_n[3] == -1 and want_c[0, 3] == 0  # the one-row group whose row is no row
            assert np.all((want_n >= -1) & (want_n < n_obs)) and want_n[1] >= 0
        run_group_mean(kern, device, f"guards: {name}", base.values, order, offsets, val_slack=2, out_slack=1, want=(want_m, want_c))
        run_group_argmin(kern, device, f"guards: {name}", base.values[0], order, offsets, want=want_n)
