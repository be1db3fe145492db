"""HEALPix ``ang2pix`` (RING and NESTED) and RING ``pix2ang`` in plain numpy / Python, and the geometry behind ``ang2pix`` exactly
(mpmath, ``PREC`` bits as tests/exact_statements.py), independent of the package.  Helper of test_healpix_host.py / test_gpu_healpix.py
and of tools/kernel_bench.py --only-healpix; holds no tests.

The float64 half is healpy's ``lonlat2thetaphi`` followed by healpix_cxx's ``ang2pix -> loc2pix`` (and ``pix2loc`` for the grid),
operation for operation (Gorski et al. 2005, ApJ 622, 759): it is what ``hp.ang2pix(nside, lon, lat, nest, lonlat=True)`` computes
(R: filters/tabular/add_healpix.py:43-51), pinned by the literals of the reference's own tests (tests/golden/healpix.json).  ``z`` and
``sth`` (cos and sin of theta) may be handed in, moved by a few ulps: the only library functions whose last bit differs between numpy and
the device.

The exact half gives the quantities the statement truncates — ``t1 -+ t2`` in the equatorial belt, ``tp * tmp``, ``(1 - tp) * tmp`` and
``tt * ir`` in the caps, and ``tt`` itself — as real geometry of the float64 inputs: z = sin(lat degrees), tt = lon / 90 mod 4, with the
true pi and no intermediate rounding.
"""

from __future__ import annotations

import json
import math
import os

import mpmath
import numpy as np

from exact_statements import PREC  # noqa: F401  (the precision mpmath.mp is set to there)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "healpix.json")
RAD = math.pi / 180.0  # np.radians multiplies by this
INV_HALFPI = 2 / math.pi
TWOTHIRD = 2.0 / 3.0
MAX_NSIDE = 1 << 29
SEED = 20051
ROWS = (1, 63, 64, 65, 257, 4099)  # the launch sizes of test_gpu_healpix.py
NEST_NSIDES, RING_NSIDES = (1, 2, 16, 1 << 29), (1, 3, 16, 1 << 29)
ULPS = 2  # sincos_moderate is held to 1 ulp from glibc; the candidate sets move z and sth by twice that


def load_golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


def npix(nside: int) -> int:
    return 12 * nside * nside


# ---- float64: ang2pix ----------------------------------------------------------------------------------------------------------
def theta_phi(lon, lat) -> tuple[np.ndarray, np.ndarray]:
    """healpy's lonlat2thetaphi."""
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    return np.pi / 2.0 - lat * RAD, lon * RAD


def valid(lon, lat) -> np.ndarray:
    """Rows that have a pixel: theta in [0, pi] (a NaN latitude is not) and a finite longitude."""
    theta, _ = theta_phi(lon, lat)
    with np.errstate(invalid="ignore"):
        return (theta >= 0.0) & (theta <= np.pi) & np.isfinite(np.asarray(lon, dtype=np.float64))


def fmodulo4(v: np.ndarray) -> np.ndarray:
    """healpix_cxx's fmodulo(v, 4.0)."""
    m = np.fmod(v, 4.0)
    neg = m + 4.0
    neg = np.where(neg == 4.0, 0.0, neg)
    return np.where(v >= 0, np.where(v < 4.0, v, m), neg)


def spread(x: np.ndarray) -> np.ndarray:
    """Bit b of x to bit 2b, bit by bit."""
    x = np.asarray(x, dtype=np.int64)
    out = np.zeros_like(x)
    for b in range(32):
        out |= ((x >> b) & 1) << (2 * b)
    return out


def parts(nside: int, lon, lat, z=None, sth=None) -> dict[str, np.ndarray]:
    """What loc2pix truncates and what it truncates it to, for valid rows: ``eq`` (equatorial region), ``tt``, ``z``, the doubles ``a``,
    ``b`` (``t1 - t2``, ``t1 + t2`` in the belt; ``tp * tmp``, ``(1 - tp) * tmp`` in the caps) with ``jp = int(a)``, ``jm = int(b)``
    (not clamped), ``ntt``, and for the caps ``c = tt * ir`` with ``ip = int(c)`` (zero in the belt)."""
    theta, phi = theta_phi(lon, lat)
    z = np.cos(theta) if z is None else np.asarray(z, dtype=np.float64)
    sth = np.sin(theta) if sth is None else np.asarray(sth, dtype=np.float64)
    za = np.abs(z)
    have_sth = (theta < 0.01) | (theta > 3.14159 - 0.01)
    tt = fmodulo4(phi * INV_HALFPI)
    eq = za <= TWOTHIRD
    dn = float(nside)
    with np.errstate(invalid="ignore"):
        t1 = dn * (0.5 + tt)
        t2 = dn * (z * 0.75)
        ntt = np.minimum(3, tt.astype(np.int64))
        tp = tt - ntt
        tmp = np.where((za < 0.99) | ~have_sth, dn * np.sqrt(3 * (1 - za)), dn * sth / np.sqrt((1.0 + za) / 3.0))
        a = np.where(eq, t1 - t2, tp * tmp)
        b = np.where(eq, t1 + t2, (1.0 - tp) * tmp)
    jp, jm = a.astype(np.int64), b.astype(np.int64)  # truncation
    ir = jp + jm + 1
    c = np.where(eq, 0.0, tt * ir)
    return dict(eq=eq, tt=tt, z=z, a=a, b=b, c=c, jp=jp, jm=jm, ntt=ntt, ip=c.astype(np.int64))


def assemble(nside: int, nest: bool, eq, jp, jm, ntt, ip, z) -> np.ndarray:
    """The pixel index from the truncated quantities: integer steps only (``z`` gives the hemisphere)."""
    eq, jp, jm, ntt, ip = (np.asarray(v) for v in (eq, jp, jm, ntt, ip))
    z = np.asarray(z, dtype=np.float64)
    nl4, ncap, n_pix = 4 * nside, 2 * nside * (nside - 1), npix(nside)
    if nest:
        if nside & (nside - 1):
            raise ValueError(f"nside {nside} is not a power of two")
        order = nside.bit_length() - 1
        ifp, ifm = jp >> order, jm >> order
        face_eq = np.where(ifp == ifm, ifp | 4, np.where(ifp < ifm, ifp, ifm + 8))
        ix_eq, iy_eq = jm & (nside - 1), nside - (jp & (nside - 1)) - 1
        cp, cm = np.minimum(jp, nside - 1), np.minimum(jm, nside - 1)
        north = z >= 0
        ix_cap, iy_cap = np.where(north, nside - cm - 1, cp), np.where(north, nside - cp - 1, cm)
        face_cap = np.where(north, ntt, ntt + 8)
        face, ix, iy = np.where(eq, face_eq, face_cap), np.where(eq, ix_eq, ix_cap), np.where(eq, iy_eq, iy_cap)
        return face * (nside * nside) + spread(ix) + 2 * spread(iy)
    ir = nside + 1 + jp - jm
    kshift = 1 - (ir & 1)
    ip_eq = ((jp + jm - nside + kshift + 1 + 8 * nside) >> 1) % nl4
    pix_eq = ncap + (ir - 1) * nl4 + ip_eq
    ir = jp + jm + 1
    pix_cap = np.where(z > 0, 2 * ir * (ir - 1) + ip, n_pix - 2 * ir * (ir + 1) + ip)
    return np.where(eq, pix_eq, pix_cap)


def ang2pix(nside: int, lon, lat, nest: bool = True, z=None, sth=None) -> np.ndarray:
    """``hp.ang2pix(nside, lon, lat, nest=nest, lonlat=True)`` as int64; -1 where ``valid`` is false."""
    lon, lat = np.asarray(lon, dtype=np.float64).reshape(-1), np.asarray(lat, dtype=np.float64).reshape(-1)
    ok = valid(lon, lat)
    out = np.full(lon.shape, -1, dtype=np.int64)
    if ok.any():
        sel = lambda v: None if v is None else np.asarray(v, dtype=np.float64).reshape(-1)[ok]  # noqa: E731
        p = parts(nside, lon[ok], lat[ok], sel(z), sel(sth))
        out[ok] = assemble(nside, nest, p["eq"], p["jp"], p["jm"], p["ntt"], p["ip"], p["z"])
    return out


def shift_ulps(x: np.ndarray, k: int) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def candidates(nside: int, lon, lat, nest: bool, ulps: int = ULPS) -> np.ndarray:
    """``[(2 ulps + 1)^2, n]``: the indices obtained with numpy's ``z`` and ``sth`` each moved by -ulps .. +ulps ulps; row
    ``len // 2`` is the unmoved statement.  Rows must be valid."""
    theta, _ = theta_phi(lon, lat)
    z, sth = np.cos(theta), np.sin(theta)
    moves = range(-ulps, ulps + 1)
    return np.stack([ang2pix(nside, lon, lat, nest, z=shift_ulps(z, dz), sth=shift_ulps(sth, ds)) for dz in moves for ds in moves])


# ---- float64: RING pix2ang and the grid ----------------------------------------------------------------------------------------------
def pix2ang_ring(nside: int, p: int) -> tuple[float, float]:
    """healpix_cxx's pix2loc + pix2ang for one RING pixel: ``(theta, phi)``."""
    n_pix, ncap = npix(nside), 2 * nside * (nside - 1)
    fact2 = 4.0 / n_pix
    fact1 = (nside << 1) * fact2
    if p < ncap or p >= n_pix - ncap:
        north = p < ncap
        if north:
            ir = (1 + math.isqrt(1 + 2 * p)) >> 1
            iphi = (p + 1) - 2 * ir * (ir - 1)
        else:
            ip = n_pix - p
            ir = (1 + math.isqrt(2 * ip - 1)) >> 1
            iphi = 4 * ir + 1 - (ip - 2 * ir * (ir - 1))
        tmp = (ir * ir) * fact2
        z = 1.0 - tmp if north else tmp - 1.0
        phi = (iphi - 0.5) * (math.pi / 2) / ir
        theta = math.atan2(math.sqrt(tmp * (2.0 - tmp)), z) if abs(z) > 0.99 else math.acos(z)
        return theta, phi
    ip = p - ncap
    ir = ip // (4 * nside) + nside
    iphi = ip % (4 * nside) + 1
    fodd = 1.0 if (ir + nside) & 1 else 0.5
    z = (2 * nside - ir) * fact1
    return math.acos(z), (iphi - fodd) * math.pi * 0.75 * fact1


def grid_point(nside: int, p: int) -> tuple[float, float]:
    """``(latitude, longitude)`` of RING pixel ``p`` as define_healpix_grid returns it (R: support/superob.py:28-40)."""
    theta, phi = pix2ang_ring(nside, p)
    lat, lon = 90 - math.degrees(theta), math.degrees(phi)
    return lat, (lon - 360 if lon > 180 else lon)


# ---- seeded cases -----------------------------------------------------------------------------------------------------------------
def random_rows(n: int, seed: int = SEED) -> tuple[np.ndarray, np.ndarray]:
    """``(lon, lat)``: latitudes uniform in sin, every fourth row within 10 degrees of a pole; longitudes in [-360, 720]."""
    rng = np.random.default_rng(seed)
    lat = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n)))
    polar = (90.0 - 10.0 * rng.uniform(0.0, 1.0, n)) * rng.choice([-1.0, 1.0], n)
    lat = np.where(np.arange(n) % 4 == 3, polar, lat)
    return rng.uniform(-360.0, 720.0, n), lat


def special_rows() -> tuple[np.ndarray, np.ndarray]:
    """``(lon, lat)``: the latitudes at which loc2pix changes branch crossed with the longitudes at which fmodulo does."""
    edge = math.degrees(math.asin(2.0 / 3.0))
    lats = [90.0, -90.0, 0.0, -0.0, np.nextafter(90.0, 0.0), np.nextafter(-90.0, 0.0)]
    for e in (edge, -edge):
        lats += [np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)]
    for theta in (0.01, 3.14159 - 0.01):  # have_sth switches here: latitudes whose theta lies just inside and just outside
        lat = (np.pi / 2.0 - theta) / RAD
        lats += [lat - 1e-9, lat + 1e-9]
    lons = [-0.0, 0.0, 45.0, 90.0, 180.0, 270.0, 360.0, 720.0, -90.0, -360.000001, 1e5, -1e5]
    lon, lat = np.meshgrid(np.array(lons), np.array(lats))
    return lon.reshape(-1).copy(), lat.reshape(-1).copy()


# ---- exact geometry ---------------------------------------------------------------------------------------------------------------
def exact_rows(lon, lat) -> list[dict]:
    """Per row, what does not depend on nside: ``tt`` = lon / 90 mod 4, ``z`` = sin(lat degrees), ``eq`` (|z| <= 2/3), ``tp`` and
    ``s`` = sqrt(3 (1 - |z|)) — mpf values, no rounding before PREC bits.  1 - |z| is taken as 2 sin^2(colatitude / 2): no cancellation."""
    out = []
    for lo, la in zip(np.asarray(lon, dtype=np.float64).tolist(), np.asarray(lat, dtype=np.float64).tolist()):
        t = mpmath.mpf(lo) / 90
        tt = t - 4 * mpmath.floor(t / 4)
        z = mpmath.sin(mpmath.mpf(la) * mpmath.pi / 180)
        za = abs(z)
        colat = mpmath.pi / 2 - abs(mpmath.mpf(la)) * mpmath.pi / 180
        s = mpmath.sqrt(6) * mpmath.sin(colat / 2)  # sqrt(3 * 2 sin^2(colat / 2))
        out.append(dict(tt=tt, z=z, za=za, eq=3 * za <= 2, tp=tt - mpmath.floor(tt), s=s))
    return out


def _gap(v) -> float:
    """Distance of an mpf from the nearest integer."""
    return float(abs(v - mpmath.nint(v)))


def exact_parts(nside: int, rows: list[dict], statement: dict | None = None) -> dict[str, np.ndarray]:
    """The exact pre-truncation values at ``nside``: their floors ``jp``, ``jm``, ``ip`` (``ip`` zero in the belt), ``ntt``, and
    ``gap``, the smallest distance of any of them from an integer; ``tt_gap`` and ``za_gap`` (|za - 2/3|) do not depend on nside.
    With ``statement`` (what ``parts`` returned for the same rows): ``off``, how far its ``a`` and ``b`` lie from the exact ones."""
    n = len(rows)
    off = np.zeros(n)
    jp, jm, ip, ntt = (np.zeros(n, dtype=np.int64) for _ in range(4))
    gap, tt_gap, za_gap, eq = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)
    two_third = mpmath.mpf(2) / 3
    for i, r in enumerate(rows):
        eq[i] = r["eq"]
        ntt[i] = int(mpmath.floor(r["tt"]))
        tt_gap[i], za_gap[i] = _gap(r["tt"]), float(abs(r["za"] - two_third))
        if r["eq"]:
            a = nside * (mpmath.mpf(0.5) + r["tt"] - r["z"] * 0.75)
            b = nside * (mpmath.mpf(0.5) + r["tt"] + r["z"] * 0.75)
            jp[i], jm[i] = int(mpmath.floor(a)), int(mpmath.floor(b))
            gap[i] = min(_gap(a), _gap(b))
        else:
            tmp = nside * r["s"]
            a, b = r["tp"] * tmp, (1 - r["tp"]) * tmp
            jp[i], jm[i] = int(mpmath.floor(a)), int(mpmath.floor(b))
            c = r["tt"] * (int(jp[i]) + int(jm[i]) + 1)
            ip[i] = int(mpmath.floor(c))
            gap[i] = min(_gap(a), _gap(b), _gap(c))
        if statement is not None and bool(statement["eq"][i]) == bool(r["eq"]):
            off[i] = float(max(abs(mpmath.mpf(float(statement["a"][i])) - a), abs(mpmath.mpf(float(statement["b"][i])) - b)))
    return dict(eq=eq, jp=jp, jm=jm, ip=ip, ntt=ntt, gap=gap, off=off, tt_gap=tt_gap, za_gap=za_gap, z=np.array([float(r["z"]) for r in rows]))
