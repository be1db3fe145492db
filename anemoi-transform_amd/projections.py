"""Vector frames of map projections: the host half of ``rotate_winds`` / ``unrotate_winds``.

The reference hands the work to pyproj and ``earthkit.geo.rotate.rotate_vector`` (R: filters/fields/rotate_winds.py:61-118).
Neither is a dependency here; this module restates the part of them that the filter needs, in float64 on the host, for a
subset of PROJ strings (``parse``).  The device applies the result (``atx_rotate_vectors_stack``, csrc/atx_rotate.hip).

Frame convention (inferred from the reference's test literals):

* the frame of ``longlat`` is local east / north on the sphere; the frame of ``ob_tran`` is the rotated grid's east / north;
  the frame of a projected CRS is its map axes (x, y);
* ``K_P`` maps a displacement given as (east, north) distance on the sphere to projection P's frame, from P's forward formulas
  (analytic derivatives); ``M(src -> tgt) = K_tgt · K_src⁻¹``;
* a vector keeps its magnitude: only its direction is mapped by ``M`` (the device statement rescales ``M w`` to ``|w|``), so K
  matters up to a positive factor per point: the frame of a conformal projection is taken with unit scale, a rotation.

For ``eqc`` with ``lat_ts = 0`` into ``longlat`` this is exactly ``diag(cos φ, 1)``, which reproduces the reference's literals.
Between two conformal projections (or longlat) ``M`` is a multiple of a rotation, and the frame is that rotation's angle.

Points at a pole (cos φ = 0) have no east / north frame: their rows of the table are not finite.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

#: the projections ``parse`` accepts (the message of its NotImplementedError)
SUPPORTED = ("longlat (aliases lonlat, latlong, latlon, EPSG:4326); eqc (lon_0, lat_ts, lat_0); ob_tran with o_proj=longlat "
             "(o_lat_p, o_lon_p, lon_0); on a sphere only (+R, or +a without b / rf / f / ellps): lcc (lat_0, lat_1, lat_2, lon_0), "
             "polar stere (lat_0 = ±90, lat_ts, lon_0), merc (lon_0, lat_ts)")
_LONGLAT = ("longlat", "lonlat", "latlong", "latlon")
#: accepted everywhere and ignored: they do not change directions
_IGNORED = ("type", "no_defs", "units", "x_0", "y_0", "to_meter", "towgs84", "datum", "k_0", "k")
_ELLIPSOID = ("R", "a", "b", "rf", "f", "ellps", "es", "e")
_KEYS = {
    "longlat": (),
    "eqc": ("lon_0", "lat_ts", "lat_0"),
    "ob_tran": ("o_proj", "o_lat_p", "o_lon_p", "lon_0"),
    "lcc": ("lat_0", "lat_1", "lat_2", "lon_0"),
    "stere": ("lat_0", "lat_ts", "lon_0"),
    "merc": ("lon_0", "lat_ts"),
}
_CONFORMAL = ("ob_tran", "lcc", "stere", "merc")
_EPS = 1e-10


@dataclass(frozen=True)
class Projection:
    """A parsed PROJ string: ``kind`` (one of ``_KEYS``) and its direction-relevant parameters in degrees."""

    kind: str
    params: dict = field(default_factory=dict, compare=False, hash=False)
    key: tuple = ()

    def p(self, name: str, default: float = 0.0) -> float:
        return float(self.params.get(name, default))

    @property
    def conformal(self) -> bool:
        """longlat counts: its frame is east / north, and every conformal frame is a rotation of it."""
        return self.kind == "longlat" or self.kind in _CONFORMAL

    # ---- lcc constants (Snyder 15-1 .. 15-3, sphere) ------------------------------------------------------------------------
    def _lcc_n(self) -> float:
        p1 = math.radians(self.p("lat_1"))
        p2 = math.radians(self.p("lat_2", self.p("lat_1")))
        if abs(p1 - p2) < _EPS:
            return math.sin(p1)
        return math.log(math.cos(p1) / math.cos(p2)) / math.log(math.tan(math.pi / 4 + p2 / 2) / math.tan(math.pi / 4 + p1 / 2))

    def _stere_akm1(self) -> float:
        ts = abs(math.radians(self.p("lat_ts", 90.0)))
        return 2.0 if abs(ts - math.pi / 2) < _EPS else math.cos(ts) / math.tan(math.pi / 4 - ts / 2)

    def _pole(self) -> tuple[float, float]:
        """ob_tran: the geographic latitude / longitude (radians) of the rotated grid's north pole."""
        return math.radians(self.p("o_lat_p", 90.0)), math.radians(self.p("lon_0") + 180.0)

    # ---- restated forward formulas (on a unit sphere; used by the tests to check the frames) -------------------------------
    def forward(self, lat, lon):
        """Projected coordinates of (lat, lon) in degrees: (lon', lat') in radians for longlat / ob_tran, map metres on a
        unit sphere otherwise (to_meter, x_0, y_0 and the radius only scale or shift them)."""
        phi, lam = np.radians(np.asarray(lat, np.float64)), np.radians(np.asarray(lon, np.float64))
        dlam = lam - math.radians(self.p("lon_0"))
        if self.kind == "longlat":
            return lam, phi
        if self.kind == "eqc":
            return dlam * math.cos(math.radians(self.p("lat_ts"))), phi - math.radians(self.p("lat_0"))
        if self.kind == "ob_tran":  # PROJ's o_forward with the pole given by o_lat_p (lon_0 subtracted first)
            sp, cp = math.sin(math.radians(self.p("o_lat_p", 90.0))), math.cos(math.radians(self.p("o_lat_p", 90.0)))
            lam_r = np.arctan2(np.cos(phi) * np.sin(dlam), sp * np.cos(phi) * np.cos(dlam) + cp * np.sin(phi))
            lam_r = lam_r + math.radians(self.p("o_lon_p"))
            return lam_r, np.arcsin(sp * np.sin(phi) - cp * np.cos(phi) * np.cos(dlam))
        if self.kind == "merc":
            k0 = math.cos(math.radians(self.p("lat_ts")))
            return k0 * dlam, k0 * np.log(np.tan(np.pi / 4 + phi / 2))
        if self.kind == "lcc":
            n = self._lcc_n()
            p1 = math.radians(self.p("lat_1"))
            F = math.cos(p1) * math.tan(math.pi / 4 + p1 / 2) ** n / n
            rho = F / np.tan(np.pi / 4 + phi / 2) ** n
            rho0 = F / math.tan(math.pi / 4 + math.radians(self.p("lat_0")) / 2) ** n
            return rho * np.sin(n * dlam), rho0 - rho * np.cos(n * dlam)
        # polar stere
        if self.p("lat_0") > 0:
            rho = self._stere_akm1() * np.tan(np.pi / 4 - phi / 2)
            return rho * np.sin(dlam), -rho * np.cos(dlam)
        rho = self._stere_akm1() * np.tan(np.pi / 4 + phi / 2)
        return rho * np.sin(dlam), rho * np.cos(dlam)

    # ---- K: (east, north) distance -> this frame, analytic ------------------------------------------------------------------
    def frame(self, lat, lon) -> np.ndarray:
        """``K`` at every point, ``[N, 2, 2]`` float64.  K matters up to a positive factor per point (the statement keeps |w|):
        conformal frames are taken with unit scale — a rotation — and eqc's is diag(cos φts / cos φ, 1) (the radius cancels)."""
        phi, lam = np.radians(np.asarray(lat, np.float64)), np.radians(np.asarray(lon, np.float64))
        dlam = lam - math.radians(self.p("lon_0"))
        K = np.zeros(phi.shape + (2, 2))
        with np.errstate(divide="ignore", invalid="ignore"):
            if self.kind == "longlat":
                K[..., 0, 0] = K[..., 1, 1] = 1.0
                return K
            if self.kind == "eqc":
                K[..., 0, 0] = math.cos(math.radians(self.p("lat_ts"))) / np.cos(phi)
                K[..., 1, 1] = 1.0
                return K
            if self.kind == "ob_tran":
                return self._ob_tran_frame(phi, lam)
        # a conformal map is its local scale times a rotation by the grid convergence γ (the angle of local east in the map's
        # axes, counter-clockwise from x): the scale is dropped, so that K is that rotation.  lcc: x = ρ sin(n Δλ), y = ρ0 - ρ cos(n Δλ) with
        # dρ/dφ = -n ρ / cos φ; polar stere: ρ = c tan(π/4 ∓ φ/2) with x = ρ sin Δλ, y = ∓ρ cos Δλ; merc: x ∝ λ, y ∝ ln tan(π/4 + φ/2).
        if self.kind == "merc":
            gamma = np.zeros_like(phi)
        elif self.kind == "lcc":
            gamma = self._lcc_n() * dlam
        else:
            gamma = dlam if self.p("lat_0") > 0 else -dlam
        c, s = np.cos(gamma), np.sin(gamma)
        K[..., 0, 0], K[..., 0, 1], K[..., 1, 0], K[..., 1, 1] = c, -s, s, c
        return K

    def frame_inverse(self, lat, lon) -> np.ndarray:
        """``K⁻¹``, in closed form: the transpose of a rotation, diag(cos φ / cos φts, 1) for eqc."""
        if self.kind == "eqc":
            K = np.zeros(np.shape(lat) + (2, 2))
            with np.errstate(divide="ignore", invalid="ignore"):
                K[..., 0, 0] = np.cos(np.radians(np.asarray(lat, np.float64))) / math.cos(math.radians(self.p("lat_ts")))
            K[..., 1, 1] = 1.0
            return K
        return np.swapaxes(self.frame(lat, lon), -1, -2).copy()

    def _ob_tran_frame(self, phi, lam) -> np.ndarray:
        """The rotated grid's east / north at P in the geographic east / north frame: east' = q × p / |q × p| (q the rotated
        pole), north' = p × east'; K holds their components (a rotation, the rotated frame being orthonormal too)."""
        pp, pl = self._pole()
        q = np.array([math.cos(pp) * math.cos(pl), math.cos(pp) * math.sin(pl), math.sin(pp)])
        cphi, sphi, clam, slam = np.cos(phi), np.sin(phi), np.cos(lam), np.sin(lam)
        p = np.stack([cphi * clam, cphi * slam, sphi], axis=-1)
        east = np.stack([-slam, clam, np.zeros_like(lam)], axis=-1)
        north = np.stack([-sphi * clam, -sphi * slam, cphi], axis=-1)
        e_r = np.cross(q, p)
        e_r = e_r / np.linalg.norm(e_r, axis=-1, keepdims=True)
        n_r = np.cross(p, e_r)
        K = np.empty(phi.shape + (2, 2))
        K[..., 0, 0] = np.sum(e_r * east, axis=-1)
        K[..., 0, 1] = np.sum(e_r * north, axis=-1)
        K[..., 1, 0] = np.sum(n_r * east, axis=-1)
        K[..., 1, 1] = np.sum(n_r * north, axis=-1)
        return K


def _number(key: str, value: str | None, text: str) -> float:
    try:
        return float(value)  # type: ignore[arg-type]
    except (TypeError, ValueError):
        raise ValueError(f"{text!r}: +{key} needs a number, got {value!r}") from None


def parse(text) -> Projection:
    """A PROJ string (or an object whose ``str()`` is one) -> ``Projection``.  A malformed string raises ValueError; a projection
    or parameter outside ``SUPPORTED`` raises NotImplementedError."""
    if isinstance(text, Projection):
        return text
    text = str(text).strip()
    if not text:
        raise ValueError("empty projection string")
    if text.upper() == "EPSG:4326":
        return Projection("longlat", {}, ("longlat",))
    code, colon, number = text.partition(":")
    if colon and code.upper() == "EPSG" and number.isdigit():
        raise NotImplementedError(f"{text!r}: EPSG codes other than 4326 are not supported (give a PROJ string); supported: {SUPPORTED}")
    values: dict[str, str | None] = {}
    for token in text.split():
        if not token.startswith("+") or len(token) == 1 or token.startswith("+="):
            raise ValueError(f"{text!r}: malformed PROJ token {token!r} (expected +key or +key=value)")
        key, eq, value = token[1:].partition("=")
        if eq and not value:
            raise ValueError(f"{text!r}: +{key}= has no value")
        if key in values:
            raise ValueError(f"{text!r}: +{key} given twice")
        values[key] = value if eq else None
    if "proj" not in values or values["proj"] is None:
        raise ValueError(f"{text!r}: no +proj=")
    kind = values.pop("proj")
    kind = "longlat" if kind in _LONGLAT else kind
    if kind not in _KEYS:
        raise NotImplementedError(f"{text!r}: projection {kind!r} is not supported; supported: {SUPPORTED}")
    if kind == "stere" and "lat_0" not in values:
        raise NotImplementedError(f"{text!r}: only polar stere (lat_0 = ±90) is supported; supported: {SUPPORTED}")
    params: dict[str, float] = {}
    for key, value in values.items():
        if key in _IGNORED or key in _ELLIPSOID:
            continue
        if key not in _KEYS[kind]:
            raise NotImplementedError(f"{text!r}: parameter +{key} is not supported for {kind}; supported: {SUPPORTED}")
        if key == "o_proj":
            if value not in _LONGLAT:
                raise NotImplementedError(f"{text!r}: ob_tran needs o_proj=longlat, got {value!r}; supported: {SUPPORTED}")
            continue
        params[key] = _number(key, value, text)
    for key in values:  # ellipsoid values must be numbers (ellps is a name)
        if key in _ELLIPSOID and key != "ellps":
            _number(key, values[key], text)
    if kind in ("lcc", "stere", "merc"):
        sphere = "R" in values or ("a" in values and not any(k in values for k in ("b", "rf", "f", "ellps", "es", "e")))
        if not sphere:
            raise NotImplementedError(
                f"{text!r}: ellipsoidal {kind} is not supported — the frame of a conformal projection on an ellipsoid differs from "
                f"the spherical one by the ellipsoid's conformal latitude, which is not restated here; give a sphere (+R=..., or +a=... "
                f"alone); supported: {SUPPORTED}")
    if kind == "ob_tran" and "o_proj" not in values:
        raise NotImplementedError(f"{text!r}: ob_tran needs o_proj=longlat; supported: {SUPPORTED}")
    if kind == "stere" and abs(abs(params.get("lat_0", 0.0)) - 90.0) > 1e-9:
        raise NotImplementedError(f"{text!r}: only polar stere (lat_0 = ±90) is supported; supported: {SUPPORTED}")
    if kind == "lcc" and "lat_1" not in params:
        raise ValueError(f"{text!r}: lcc needs +lat_1")
    if kind == "lcc" and abs(Projection(kind, params)._lcc_n()) < _EPS:
        raise ValueError(f"{text!r}: lcc with standard parallels symmetric about the equator has no cone (n = 0)")
    if kind == "ob_tran":  # o_lon_p does not change directions: only the pole does
        key = (kind, params.get("o_lat_p", 90.0), params.get("lon_0", 0.0) % 360.0)
    elif kind == "eqc":
        key = (kind, abs(params.get("lat_ts", 0.0)))
    elif kind == "lcc":
        key = (kind, params.get("lat_1"), params.get("lat_2", params.get("lat_1")), params.get("lon_0", 0.0) % 360.0)
    elif kind == "stere":
        key = (kind, math.copysign(90.0, params["lat_0"]), params.get("lon_0", 0.0) % 360.0)
    else:
        key = (kind,)
    return Projection(kind, params, key)


def matrix(lats, lons, src, tgt) -> np.ndarray:
    """``M(src -> tgt) = K_tgt · K_src⁻¹`` at every point, ``[N, 2, 2]`` float64."""
    src, tgt = parse(src), parse(tgt)
    return np.einsum("...ij,...jk->...ik", tgt.frame(lats, lons), src.frame_inverse(lats, lons))


def vector_frame(lats, lons, src, tgt) -> tuple[str, np.ndarray]:
    """The per-point table of ``atx_rotate_vectors_stack``: ``("rotation", [N, 2] = cos γ, sin γ)`` when both sides are
    conformal or longlat, else ``("general", [N, 4] = m00, m01, m10, m11)``; float64."""
    src, tgt = parse(src), parse(tgt)
    lats = np.asarray(lats, np.float64).reshape(-1)
    lons = np.asarray(lons, np.float64).reshape(-1)
    M = matrix(lats, lons, src, tgt)
    if src.conformal and tgt.conformal:
        gamma = np.arctan2(M[:, 1, 0] - M[:, 0, 1], M[:, 0, 0] + M[:, 1, 1])
        return "rotation", np.stack([np.cos(gamma), np.sin(gamma)], axis=1)
    return "general", M.reshape(-1, 4).copy()


def apply_frame(kind: str, frame: np.ndarray, u: np.ndarray, v: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The statement of ``atx_rotate_vectors_stack`` in numpy, in the dtype of ``u`` / ``v`` (the frame cast to it), no fma:
    rotation ``(c u − s v, s u + c v)``; general ``mx = m00 u + m01 v``, ``my = m10 u + m11 v``,
    ``k = sqrt(u u + v v) / sqrt(mx mx + my my)``, ``(mx k, my k)``; a zero vector (u == v == 0) is returned as it is.
    ``frame`` is ``[N, F]`` and broadcasts over leading level axes of ``u`` / ``v`` (``[..., N]``)."""
    dt = u.dtype
    f = np.asarray(frame).astype(dt)
    with np.errstate(all="ignore"):
        if kind == "rotation":
            c, s = f[:, 0], f[:, 1]
            x, y = c * u - s * v, s * u + c * v
        else:
            mx = f[:, 0] * u + f[:, 1] * v
            my = f[:, 2] * u + f[:, 3] * v
            k = np.sqrt(u * u + v * v) / np.sqrt(mx * mx + my * my)
            x, y = mx * k, my * k
    zero = (u == 0) & (v == 0)
    return np.where(zero, u, x).astype(dt), np.where(zero, v, y).astype(dt)


#: what earthkit-data's Field.projection() gives for a regular latitude / longitude grid (the reference's tests use it)
REGULAR_LATLON = "+proj=eqc +ellps=WGS84 +a=6378137.0 +lon_0=0.0 +to_meter=111319.4907932736 +no_defs +type=crs"
