"""HEALPix: pixel indices of observation rows on the device, and the RING-ordered grid of a resolution.

``ang2pix`` is healpy's ``hp.ang2pix(nside, lon, lat, nest, lonlat=True)`` (R: filters/tabular/add_healpix.py:43-51) as ONE launch of
``atx_healpix_ang2pix`` over columns that stay in HBM; ``grid`` is the reference's ``define_healpix_grid``
(R: filters/tabular/support/superob.py:28-40), the points an ``"h<nside>"`` grid name stands for.  healpy itself is not used: the
pixelisation is a closed-form statement (Gorski et al. 2005, ApJ 622, 759; healpix_cxx ``loc2pix`` / ``pix2loc``), restated in float64
in the operation order of the source and pinned by the literals of the reference's own tests (tests/golden/healpix.json).

Parity: away from pixel edges the index is the exact geometry's.  On an edge the last bit of cos / sin of the colatitude decides between
the two neighbouring pixels, and the device's cos / sin may differ from glibc's in that bit (``sincos_moderate``, < 1 ulp).
"""

from __future__ import annotations

import logging
from typing import Any

import numpy as np
import torch

from . import native, obs
from . import stack as _stack
from .core import say_once

LOG = logging.getLogger(__name__)

MAX_NSIDE = 1 << 29


def check_nside(nside: Any, nest: bool = False) -> int:
    """``nside`` as an int in 1 .. 2^29, for the NESTED ordering a power of two (healpy's ``check_nside``); ``ValueError`` otherwise."""
    if isinstance(nside, bool) or not isinstance(nside, (int, np.integer)) or not 1 <= nside <= MAX_NSIDE:
        raise ValueError(f"nside must be an integer in 1 .. 2^29, got {nside!r}")
    if nest and nside & (nside - 1):
        raise ValueError(f"{nside} is not a valid nside parameter (must be a power of 2, less than 2**30)")  # healpy's check_nside
    return int(nside)


def parity_note() -> None:
    """Said once per process, by the first ``ang2pix`` or the first ``add_healpix`` filter: what the indices are held to."""
    say_once(LOG, "healpix-parity", "healpix: healpy's ang2pix is restated (healpix_cxx loc2pix in float64), not called; it is pinned by "
             "the reference's nine literals and held to the exact geometry away from pixel edges; on an edge the last bit of cos / sin "
             "decides between the two neighbouring pixels")


def npix(nside: int) -> int:
    """``12 * nside**2``, the number of pixels (``hp.nside2npix``)."""
    return 12 * check_nside(nside) ** 2


def ang2pix(nside: int, longitude: Any, latitude: Any, *, nest: bool = True, dev: torch.device | None = None) -> torch.Tensor:
    """The HEALPix pixel of every ``(longitude, latitude)`` in degrees, as an int64 device tensor — ``atx_healpix_ang2pix``.

    ``nest=True`` (the ``add_healpix`` filter's): NESTED ordering, ``nside`` a power of two; ``nest=False``: RING ordering, any
    ``nside``.  Columns are numpy arrays, pandas Series or device tensors; they are read as float64 (a float64 device tensor is used in
    place).  A NaN latitude, a latitude outside [-90, 90] or a longitude that is not finite has no pixel: ``ValueError`` naming how
    many such rows there are (synchronises)."""
    nside = check_nside(nside, nest)
    dev = _stack.device() if dev is None else dev
    lon, lat = obs.float_column(longitude, dev), obs.float_column(latitude, dev)
    if lon.numel() != lat.numel():
        raise ValueError(f"columns differ in length: longitude {lon.numel()}, latitude {lat.numel()}")
    parity_note()
    out = torch.empty(lon.numel(), dtype=torch.int64, device=dev)
    n_bad = torch.zeros(1, dtype=torch.int64, device=dev)
    native.healpix_ang2pix(lon, lat, nside, nest, out, n_bad)
    bad = int(n_bad.item())
    if bad:
        raise ValueError(f"healpix: {bad} of {lon.numel()} rows have no pixel (latitude NaN or outside [-90, 90], or a longitude that "
                         "is not finite)")
    return out


def _isqrt(v: np.ndarray) -> np.ndarray:
    r = np.sqrt(v.astype(np.float64)).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)
    return np.where((r + 1) * (r + 1) <= v, r + 1, r)


def pix2ang_ring(nside: int, pix: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
    """``hp.pix2ang(nside, pix)`` for RING-ordered pixels (all of them by default): ``(theta, phi)`` in radians, float64, host arrays
    (healpix_cxx ``pix2loc``)."""
    nside = check_nside(nside)
    n_pix, ncap, nl4 = 12 * nside * nside, 2 * nside * (nside - 1), 4 * nside
    p = np.arange(n_pix, dtype=np.int64) if pix is None else np.asarray(pix, dtype=np.int64).reshape(-1)
    if p.size and (p.min() < 0 or p.max() >= n_pix):
        raise ValueError(f"pixel indices outside 0 .. {n_pix - 1}")
    fact2 = 4.0 / n_pix
    fact1 = (nside << 1) * fact2
    north, south = p < ncap, p >= n_pix - ncap
    cap = north | south
    # the caps, the southern one mirrored
    ip = np.where(north, p, n_pix - p)
    ir = np.where(north, (1 + _isqrt(1 + 2 * ip)) >> 1, (1 + _isqrt(np.maximum(2 * ip - 1, 0))) >> 1)
    ir = np.maximum(ir, 1)  # belt rows, unused
    iphi = np.where(north, (ip + 1) - 2 * ir * (ir - 1), 4 * ir + 1 - (ip - 2 * ir * (ir - 1)))
    tmp = (ir * ir) * fact2
    z_cap = np.where(north, 1.0 - tmp, tmp - 1.0)
    phi_cap = (iphi - 0.5) * (np.pi / 2) / ir
    with np.errstate(invalid="ignore"):
        theta_cap = np.where(np.abs(z_cap) > 0.99, np.arctan2(np.sqrt(tmp * (2.0 - tmp)), z_cap), np.arccos(np.clip(z_cap, -1.0, 1.0)))
    # the belt
    ib = p - ncap
    irb = ib // nl4 + nside
    iphib = ib % nl4 + 1
    fodd = np.where((irb + nside) & 1, 1.0, 0.5)
    z_belt = (2 * nside - irb) * fact1
    theta_belt = np.arccos(np.clip(z_belt, -1.0, 1.0))
    phi_belt = (iphib - fodd) * np.pi * 0.75 * fact1
    return np.where(cap, theta_cap, theta_belt), np.where(cap, phi_cap, phi_belt)


def grid(nside: int) -> tuple[np.ndarray, np.ndarray]:
    """``(latitudes, longitudes)`` of the ``12 * nside**2`` pixel centres in RING order, longitudes above 180 reduced by 360 — the
    reference's ``define_healpix_grid`` (R: support/superob.py:28-40).  Host arrays, as every grid of this package."""
    theta, phi = pix2ang_ring(nside)
    lat = 90 - np.degrees(theta)
    lon = np.degrees(phi)
    return lat, np.where(lon > 180, lon - 360, lon)
