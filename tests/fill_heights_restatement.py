"""The ``fill_orography`` filter stated in numpy and scipy, independent of the package, with the seeded inputs its tests share.

The statement: a row whose station altitude is NaN or exactly 9999.0 gets ``heights[i, j]``, where ``i`` is what a ``cKDTree`` over the
orography's latitude axis (one coordinate per point) answers for the row's latitude and ``j`` the same for the longitudes; every other
row keeps its altitude.  A tree over one coordinate returns the entry with the smallest float64 ``(a - q) * (a - q)``; which entry it
returns when two are equally near depends on how the tree was built, so ``ties`` says for which rows that is the case: there only the
tree itself is an authority (tests/golden/fill_heights.json records the reference's answers for a block of such rows).
"""

from __future__ import annotations

import json
import os

import numpy as np
from scipy.spatial import cKDTree

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fill_heights.json")
SENTINEL = 9999.0
ROWS = (1, 63, 64, 65, 255, 256, 257, 4099)  # wave and block edges, a partial last block, more than one block
SHAPES = ((1, 1), (2, 3), (181, 360))
KINDS = ("ascending", "descending", "shuffled")
TIE_LATITUDE, TIE_LONGITUDE = 1, 2


# ---- the statement ------------------------------------------------------------------------------------------------------------------
def to_fill(stalt: np.ndarray) -> np.ndarray:
    stalt = np.asarray(stalt, dtype=np.float64)
    return np.isnan(stalt) | (stalt == SENTINEL)


def nearest(axis: np.ndarray, q: np.ndarray) -> np.ndarray:
    """What the tree over ``axis`` answers for every ``q``."""
    _, index = cKDTree(np.asarray(axis, dtype=np.float64).reshape(-1, 1)).query(np.asarray(q, dtype=np.float64).reshape(-1, 1))
    return index


def fill(lat_axis, lon_axis, heights, latitude, longitude, stalt) -> np.ndarray:
    """The filled altitude column, float64."""
    out = np.array(stalt, dtype=np.float64)
    rows = np.flatnonzero(to_fill(out))
    lat, lon = np.asarray(latitude, dtype=np.float64)[rows], np.asarray(longitude, dtype=np.float64)[rows]
    out[rows] = np.asarray(heights)[nearest(lat_axis, lat), nearest(lon_axis, lon)]
    return out


def ties(axis: np.ndarray, q: np.ndarray) -> np.ndarray:
    """Per ``q``: more than one entry of ``axis`` attains the smallest float64 square, so the tree's answer is an artefact of its build."""
    axis, q = np.asarray(axis, dtype=np.float64), np.asarray(q, dtype=np.float64)
    out = np.empty(q.size, dtype=bool)
    with np.errstate(over="ignore"):
        for start in range(0, q.size, 1024):
            d = axis[:, None] - q[None, start:start + 1024]
            d2 = d * d
            out[start:start + 1024] = (d2 == d2.min(axis=0)).sum(axis=0) > 1
    return out


def tie_bits(lat_axis, lon_axis, latitude, longitude, stalt) -> np.ndarray:
    """uint8 per row: ``TIE_LATITUDE`` / ``TIE_LONGITUDE`` where a row to fill has a tie on that axis, 0 for kept rows."""
    fill_rows = to_fill(stalt)
    bits = np.where(ties(lat_axis, latitude), TIE_LATITUDE, 0) | np.where(ties(lon_axis, longitude), TIE_LONGITUDE, 0)
    return np.where(fill_rows, bits, 0).astype(np.uint8)


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------
def axes(kind: str, n_lat: int = 181, n_lon: int = 360, seed: int = 7) -> tuple[np.ndarray, np.ndarray]:
    """``(latitudes, longitudes)`` of a regular global grid of ``n_lat x n_lon`` points in the order ``kind`` names."""
    lat = np.linspace(-90.0, 90.0, n_lat) if n_lat > 1 else np.array([12.5])
    lon = np.arange(n_lon) * (360.0 / n_lon) if n_lon > 1 else np.array([33.0])
    if kind == "descending":
        return lat[::-1].copy(), lon[::-1].copy()
    if kind == "shuffled":
        rng = np.random.default_rng(seed)
        return rng.permutation(lat), rng.permutation(lon)
    assert kind == "ascending", kind
    return lat, lon


def heights(n_lat: int, n_lon: int, dtype=np.float32, seed: int = 11) -> np.ndarray:
    """Distinct values per cell, so that a wrong index shows; float32 values are not all float64-round numbers."""
    rng = np.random.default_rng(seed)
    h = (rng.uniform(-400.0, 8800.0, (n_lat, n_lon)) + np.arange(n_lat * n_lon).reshape(n_lat, n_lon) * 1e-3).astype(dtype)
    h.flat[0] = -0.0
    return h


def rows(n: int, seed: int = 20261019) -> dict[str, np.ndarray]:
    """``latitude``, ``longitude``, ``stalt`` of ``n`` rows: coordinates partly beyond the axes' ends (latitude in [-95, 95], longitude
    in [-20, 400]); about a quarter of the altitudes NaN, a quarter 9999.0, the rest kept values."""
    rng = np.random.default_rng(seed)
    lat, lon = rng.uniform(-95.0, 95.0, n), rng.uniform(-20.0, 400.0, n)
    kind = rng.integers(0, 4, n)
    stalt = rng.uniform(-400.0, 8800.0, n)
    stalt[kind == 0] = np.nan
    stalt[kind == 1] = SENTINEL
    return {"latitude": lat, "longitude": lon, "stalt": stalt}


def midpoint_axes() -> tuple[np.ndarray, np.ndarray]:
    """One-degree axes, small enough for the golden file: latitudes -10 .. 10, longitudes 0 .. 29."""
    return np.arange(-10.0, 11.0), np.arange(0.0, 30.0)


def midpoint_rows() -> dict[str, np.ndarray]:
    """Rows exactly half-way between two entries of ``midpoint_axes``: on both axes, on the latitudes only, on the longitudes only.
    Every row is to fill (NaN and the sentinel alternate)."""
    lat_mid, lon_mid = np.arange(-10.0, 10.0) + 0.5, np.arange(0.0, 29.0) + 0.5
    lat = np.concatenate([np.resize(lat_mid, 29), lat_mid, np.full(29, 3.25)])
    lon = np.concatenate([lon_mid, np.full(20, 7.25), lon_mid])
    stalt = np.where(np.arange(lat.size) % 2 == 0, np.nan, SENTINEL)
    return {"latitude": lat, "longitude": lon, "stalt": stalt}


# ---- the golden file ----------------------------------------------------------------------------------------------------------------
def encode(a) -> dict:
    """An array as its dtype, shape and integer bit patterns: equality of what comes back is exact, NaN payloads and -0.0 included."""
    a = np.ascontiguousarray(a)
    bits = a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
    return {"dtype": a.dtype.name, "shape": list(a.shape), "bits": bits.reshape(-1).tolist()}


def decode(spec: dict) -> np.ndarray:
    dtype = np.dtype(spec["dtype"])
    store = {4: np.int32, 8: np.int64}[dtype.itemsize] if dtype.kind == "f" else dtype
    return np.array(spec["bits"], dtype=store).view(dtype).reshape(spec["shape"])


def load_golden() -> list[dict]:
    """The recorded cases with their arrays decoded: ``lat_axis``, ``lon_axis``, ``heights``, ``table`` (name -> column), ``expected`` (the
    frame's altitude column), ``direct`` (``get_heights`` for the rows to fill), ``config`` and ``id``."""
    with open(GOLDEN) as f:
        cases = json.load(f)["cases"]
    for case in cases:
        for key in ("lat_axis", "lon_axis", "heights", "expected", "direct"):
            case[key] = decode(case[key])
        case["table"] = {name: decode(spec) for name, spec in case["table"].items()}
    return cases


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
