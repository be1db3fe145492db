"""The four per-row observation filters in plain numpy, and exactly (mpmath, ``PREC`` bits as tests/exact_statements.py), independent of
the package (R: filters/tabular/add_forcings.py, add_azimuth.py, add_msg_angles.py, radiance_to_brightness_temperature.py,
support/compute_forcings.py, support/sat_view_angles.py).  Helper of test_obs_rowops_host.py / test_gpu_obs_rowops.py and of
tools/record_rowops_golden.py; holds no tests.

The numpy half restates the statements operation for operation — what the reference's pandas calls come to on int64 nanoseconds and
float64 columns — so it equals the frames the reference's own modules returned (tests/golden/obs_rowops.json) bit for bit.  The exact
half evaluates the same statements without rounding, every literal (``np.pi``, ``pi / 180``, the coefficients) as the float64 the
source holds.  Two kinds of exact reference, as in exact_statements.py: the eight single-function forcings are the exact cos / sin of
the argument AS THE STATEMENT ROUNDS IT (``forcing_arguments``); ``cos_sza``, azimuth, zenith and the brightness temperature are the
whole statement, exact from the inputs.
"""

from __future__ import annotations

import json
import math
import os
import re

import mpmath
import numpy as np

from exact_statements import PREC, ulp_errors  # noqa: F401  (PREC: the precision mpmath.mp is set to there)
from superob_restatement import decode_column, encode_column  # noqa: F401  (columns as int64 bit patterns)

NAT = np.iinfo(np.int64).min
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obs_rowops.json")
FORCINGS = ("cos_julian_day", "sin_julian_day", "cos_sza", "sin_local_time", "cos_local_time", "cos_latitude", "sin_latitude",
            "cos_longitude", "sin_longitude")  # R: add_forcings.py:51-61
SINGLE_FORCINGS = tuple(c for c in FORCINGS if c != "cos_sza")
RAD, DEG = math.pi / 180.0, 180.0 / math.pi  # np.deg2rad / np.radians and np.degrees multiply by these
NS_DAY, NS_SECOND = 86400 * 10**9, 10**9

# numpy's own worst error against the exact statements on the generators below (3000 cases, seed 0): cos_sza in units of 2^-53,
# azimuth and zenith in ulps of 360 (azimuth: circular distance), the brightness temperature in ulps.  Pinned within
# [0.8 x, 1.1 x + 0.1] by test_obs_rowops_host.py; the kernels' ceilings are 2 x + SLACK (every device library function is specified at up
# to 2 ulps where glibc's stay within 1, and the statement amplifies both alike).
NUMPY_WORST = {"cos_sza": 9.78, "azimuth": 15.35, "zenith": 1.25, "brightness_temperature": 1.86}
SLACK = 2.0
CEILING = {name: 2.0 * NUMPY_WORST[name] + SLACK for name in ("cos_sza", "azimuth", "zenith")}
CEILING["brightness_temperature"] = 3.0  # R * 1e-2 and a / R: 0.5 each through log1p (condition <= 1), log1p 1, b / . 0.5
SINCOS_BUDGET = 1.0  # the eight single-function forcings: the library's own sincos routine (|x| < 1e5)
U53 = 2.0**-53
ULP360 = float(np.spacing(360.0))


# ---- the calendar -------------------------------------------------------------------------------------------------------------
def to_ns(date) -> np.ndarray:
    a = np.asarray(date)
    return a.astype(np.int64) if a.dtype.kind == "i" else a.astype("datetime64[ns]").view(np.int64)


def julian_day_and_hours(date) -> tuple[np.ndarray, np.ndarray]:
    """``delta.days + delta.seconds / 86400.0`` from the start of the date's year, and ``(delta.seconds / 86400.0) * 24`` from the start
    of its day (R: add_forcings.py:99-114): WHOLE days and seconds, NaN for NaT."""
    ns = to_ns(date)
    ok = ns != NAT
    safe = np.where(ok, ns, 0)
    days = safe // NS_DAY  # floor: dates before 1970
    seconds = (safe - days * NS_DAY) // NS_SECOND
    year_start = safe.view("datetime64[ns]").astype("datetime64[Y]").astype("datetime64[D]").astype(np.int64)
    fraction = seconds / 86400.0
    julian_day = (days - year_start) + fraction
    hours = (0 + fraction) * 24
    return np.where(ok, julian_day, np.nan), np.where(ok, hours, np.nan)


# ---- forcings -------------------------------------------------------------------------------------------------------------------
def forcing_arguments(date, latitude, longitude) -> dict[str, np.ndarray]:
    """The radians each single-function forcing takes the cos / sin of, rounded as the statement rounds them (R: add_forcings.py:86-127)."""
    julian_day, hours = julian_day_and_hours(date)
    latitude, longitude = np.asarray(latitude, dtype=np.float64), np.asarray(longitude, dtype=np.float64)
    with np.errstate(all="ignore"):
        local_time = (longitude / 360.0 * 24.0 + hours) % 24
        return {"julian_day": julian_day / 365.25 * np.pi * 2, "local_time": local_time / 24 * np.pi * 2,
                "latitude": np.deg2rad(latitude), "longitude": np.deg2rad(longitude)}


def cos_solar_zenith_angle(julian_days, hours, latitudes, longitudes) -> np.ndarray:
    """R: support/compute_forcings.py:14-87, statement for statement."""
    angle = julian_days / 365.25 * np.pi * 2
    declination = (0.396372 - 22.91327 * np.cos(angle) + 4.025430 * np.sin(angle) - 0.387205 * np.cos(2 * angle) + 0.051967 * np.sin(2 * angle)
                   - 0.154527 * np.cos(3 * angle) + 0.084798 * np.sin(3 * angle))
    time_correction = (0.004297 + 0.107029 * np.cos(angle) - 1.837877 * np.sin(angle) - 0.837378 * np.cos(2 * angle)
                       - 2.340475 * np.sin(2 * angle))
    declination = np.deg2rad(declination)
    latitudes = np.deg2rad(latitudes)
    sindec_sinlat = np.sin(declination) * np.sin(latitudes)
    cosdec_coslat = np.cos(declination) * np.cos(latitudes)
    solar_angle = np.deg2rad((hours - 12) * 15 + longitudes + time_correction)
    zenith_angle = sindec_sinlat + cosdec_coslat * np.cos(solar_angle)
    return np.clip(zenith_angle, 0, None)


def forcings(date, latitude, longitude, columns) -> dict[str, np.ndarray]:
    latitude, longitude = np.asarray(latitude, dtype=np.float64), np.asarray(longitude, dtype=np.float64)
    args = forcing_arguments(date, latitude, longitude)
    out = {}
    with np.errstate(all="ignore"):
        for column in columns:
            if column == "cos_sza":
                out[column] = cos_solar_zenith_angle(*julian_day_and_hours(date), latitude, longitude)
                continue
            fn, variable = column.split("_", maxsplit=1)
            out[column] = getattr(np, fn)(args[variable])
    return out


# ---- view angles ----------------------------------------------------------------------------------------------------------------
def calc_zenith(latdeg, londeg, satlats, satlons) -> np.ndarray:
    """R: support/sat_view_angles.py:17-49."""
    rearth = 6378.170
    satalt = 6610839 * 1.0e-6 * rearth - rearth
    rsatlons, rsatlats, rlons, rlats = np.radians(satlons), np.radians(satlats), np.radians(londeg), np.radians(latdeg)
    with np.errstate(all="ignore"):
        ds = rearth * 2 * np.arcsin(np.sqrt((1 - np.sin(rlats) * np.sin(rsatlats) - np.cos(rlats) * np.cos(rsatlats) * np.cos(rlons - rsatlons)) / 2))
        a = ds / rearth
        rl = rearth * np.sin(a)
        rm = rearth * np.cos(a)
        tb = rl / (rearth + satalt - rm)
        return np.degrees(a + np.arctan(tb))


def azimuth_mask(latdeg, londeg, satlats, satlons) -> np.ndarray:
    with np.errstate(all="ignore"):
        return (np.abs(latdeg - satlats) > 0.00001) & (np.abs(londeg - satlons) > 0.00001)


def calc_azimuth(latdeg, londeg, satlats, satlons) -> np.ndarray:
    """R: support/sat_view_angles.py:52-97."""
    latdeg, londeg = np.asarray(latdeg, dtype=np.float64), np.asarray(londeg, dtype=np.float64)
    satlats, satlons = np.asarray(satlats, dtype=np.float64), np.asarray(satlons, dtype=np.float64)
    azm = np.zeros_like(latdeg)
    mask = azimuth_mask(latdeg, londeg, satlats, satlons)
    lat, lon, latS, lonS = np.radians(latdeg[mask]), np.radians(londeg[mask]), np.radians(satlats[mask]), np.radians(satlons[mask])
    with np.errstate(all="ignore"):
        zdlon = lonS - lon
        zdlat = latS - lat
        za = np.sin(zdlat / 2.0) ** 2 + np.cos(lat) * np.cos(latS) * np.sin(zdlon / 2.0) ** 2
        distOS = 2.0 * np.arcsin(np.minimum(1.0, np.sqrt(za)))
        azmsin = np.cos(latS) / np.sin(distOS) * np.sin(lon - lonS)
        azmsin = np.arcsin(np.clip(azmsin, -1.0, 1.0))
        azmcos = (np.sin(latS) - np.sin(lat) * np.cos(distOS)) / (np.cos(lat) * np.sin(distOS))
        azmcos = np.arccos(np.clip(azmcos, -1.0, 1.0))
        azmcos = np.where(azmsin > 0, -azmcos, azmcos)
        azm_calc = np.where(azmcos >= np.pi, azmcos - 2.0 * np.pi, azmcos)
        azm_calc = np.where(azm_calc < -np.pi, azm_calc + 2.0 * np.pi, azm_calc)
        azm[mask] = np.mod(np.degrees(azm_calc), 360.0)
    return azm


THRESHOLDS = {55: ("2016-10-20", ">", 41.5), 56: ("2022-05-08", ">", 45.5), 57: ("2013-01-24", "<", -3.4), 70: ("2015-12-01", "<", -3.4)}


def meteosat_loc(satids, date) -> tuple[np.ndarray, np.ndarray]:
    """R: support/sat_view_angles.py:100-132 — the tables take the DTYPE OF THE ID COLUMN (``np.zeros_like(satids)``): integer ids
    store 41.5 / 45.5 / -3.4 as 41 / 45 / -3.  Strict comparisons; NaT compares false."""
    satids = np.asarray(satids)
    ns = to_ns(date)
    lons, lats = np.zeros_like(satids), np.zeros_like(satids)
    for sat, (day, side, lon) in THRESHOLDS.items():
        limit = int(np.datetime64(day, "ns").astype(np.int64))
        when = (ns > limit) if side == ">" else (ns < limit)
        lons[(satids == sat) & when & (ns != NAT)] = lon
    return lats, lons


# ---- brightness temperature -------------------------------------------------------------------------------------------------------
C1_W, C2 = 1.191042e-10, 1.4387768775
BANDS = {"cris_fsr": ((1, 713, 650.0, 0.625), (714, 1578, 1210.0, 0.625), (1579, 2211, 2155.0, 0.625)),
         "cris_nsr": ((1, 713, 650.0, 0.625), (714, 1146, 1210.0, 1.250), (1147, 1305, 2155.0, 2.500))}


def wavenumbers(channels, mode: str) -> np.ndarray:
    """R: radiance_to_brightness_temperature.py:52-80; NaN outside the bands."""
    ch = np.asarray(channels, dtype=np.int64)
    nu = np.full(ch.shape, np.nan, dtype=float)
    for first, last, start, step in BANDS[mode]:
        m = (first <= ch) & (ch <= last)
        nu[m] = start + step * (ch[m] - first)
    return nu


def planck_tables(channels, mode: str) -> tuple[np.ndarray, np.ndarray]:
    nu = wavenumbers(channels, mode)
    return C1_W * (nu**3), C2 * nu


def brightness_temperature(radiance, a, b) -> np.ndarray:
    """``radiance``: [n_rows, n_ch]; ``a``, ``b``: [n_ch] (R: :111-113)."""
    with np.errstate(all="ignore"):
        R = np.asarray(radiance, dtype=float) * 1e-2
        return b / np.log1p(a / np.maximum(R, 1e-300))


def radiance_columns(names, prefix: str) -> tuple[list[str], np.ndarray]:
    """The columns starting with ``prefix`` sorted by their trailing channel number, and the numbers (R: :84-94)."""
    cols = [c for c in names if str(c).startswith(prefix)]
    chans = np.array([int(re.search(r"_(\d+)$", c).group(1)) for c in cols], dtype=np.int64)
    order = np.argsort(chans)
    return [cols[i] for i in order], chans[order]


# ---- the four filters on a dict of columns ----------------------------------------------------------------------------------------
def apply_filter(name: str, config: dict, table: dict) -> dict:
    """What the reference's filter returns for ``table`` (a dict ``name -> array``), as a dict in the frame's column order."""
    out = dict(table)
    if name == "add_forcings":
        out.update(forcings(table["date"], table["latitude"], table["longitude"], config["columns"]))
    elif name == "add_azimuth":
        sc_lat, sc_lon = config.get("spacecraft_latitude", "spacecraft_latitude"), config.get("spacecraft_longitude", "spacecraft_longitude")
        out[config.get("azimuth", "azimuth")] = calc_azimuth(table["latitude"], table["longitude"], table[sc_lat], table[sc_lon])
    elif name == "add_msg_angles":
        lats, lons = meteosat_loc(table[config.get("satellite_id", "satellite_id")], table["date"])
        angle = config.get("angle", "both")
        if angle in ("azimuth", "both"):
            out[config.get("azimuth", "azimuth")] = calc_azimuth(table["latitude"], table["longitude"], lats, lons)
        if angle in ("zenith", "both"):
            out[config.get("zenith", "zenith")] = calc_zenith(np.asarray(table["latitude"], dtype=np.float64),
                                                              np.asarray(table["longitude"], dtype=np.float64), lats, lons)
    else:
        assert name == "radiance_to_brightness_temperature", name
        prefix, out_prefix = config.get("input_prefix", "obsvalue_rad_"), config.get("output_prefix", "obsvalue_rawbt_")
        cols, chans = radiance_columns(list(table), prefix)
        a, b = planck_tables(chans, config["mode"])
        tb = brightness_temperature(np.column_stack([np.asarray(table[c], dtype=float) for c in cols]), a, b)
        new = {c: (f"{out_prefix}{ch}", tb[:, j]) for j, (c, ch) in enumerate(zip(cols, chans))}
        out = {}
        for c, v in table.items():
            key, val = new.get(c, (c, v))
            out[key] = val
    return out


# ---- exact statements ---------------------------------------------------------------------------------------------------------------
m = mpmath.mpf
PI, TWO_PI = m(math.pi), m(2.0 * math.pi)  # np.pi and 2.0 * np.pi, the float64 values the statements hold


def _finite(*xs) -> bool:
    return all(math.isfinite(x) for x in xs)


def cos_exact(a: float):
    return math.nan if not math.isfinite(a) else mpmath.cos(m(a))


def sin_exact(a: float):
    if not math.isfinite(a):
        return math.nan
    return a if a == 0 else mpmath.sin(m(a))


def cos_sza_exact(julian_day: float, hours: float, latitude: float, longitude: float):
    """The whole statement, unclipped (the caller clips: a negative value gives exactly 0.0)."""
    if not _finite(julian_day, hours, latitude, longitude):
        return math.nan
    angle = m(julian_day) / m(365.25) * PI * 2
    c1, s1, c2, s2, c3, s3 = (f(k * angle) for k in (1, 2, 3) for f in (mpmath.cos, mpmath.sin))
    declination = (m(0.396372) - m(22.91327) * c1 + m(4.025430) * s1 - m(0.387205) * c2 + m(0.051967) * s2 - m(0.154527) * c3 + m(0.084798) * s3)
    time_correction = m(0.004297) + m(0.107029) * c1 - m(1.837877) * s1 - m(0.837378) * c2 - m(2.340475) * s2
    declination = declination * m(RAD)
    lat = m(latitude) * m(RAD)
    solar_angle = ((m(hours) - 12) * 15 + m(longitude) + time_correction) * m(RAD)
    return mpmath.sin(declination) * mpmath.sin(lat) + mpmath.cos(declination) * mpmath.cos(lat) * mpmath.cos(solar_angle)


def zenith_exact(latdeg: float, londeg: float, satlat: float, satlon: float):
    if not _finite(latdeg, londeg, satlat, satlon):
        return math.nan
    rearth = m(6378.170)
    satalt = m(6610839) * m(1.0e-6) * rearth - rearth
    lat, lon, latS, lonS = (m(x) * m(RAD) for x in (latdeg, londeg, satlat, satlon))
    inner = (1 - mpmath.sin(lat) * mpmath.sin(latS) - mpmath.cos(lat) * mpmath.cos(latS) * mpmath.cos(lon - lonS)) / 2
    a = 2 * mpmath.asin(mpmath.sqrt(max(inner, m(0))))
    tb = rearth * mpmath.sin(a) / (rearth + satalt - rearth * mpmath.cos(a))
    return (a + mpmath.atan(tb)) * m(DEG)


def azimuth_exact(latdeg: float, londeg: float, satlat: float, satlon: float):
    """``(azimuth, sine term)``: the exact statement on a row that passes the mask, and the exact ``azmsin`` before its clip, whose
    sign decides the switch — within 1e-12 of 0 the statement jumps and a row may be left out of the ulp comparison."""
    lat, lon, latS, lonS = (m(x) * m(RAD) for x in (latdeg, londeg, satlat, satlon))
    za = mpmath.sin((latS - lat) / 2) ** 2 + mpmath.cos(lat) * mpmath.cos(latS) * mpmath.sin((lonS - lon) / 2) ** 2
    dist = 2 * mpmath.asin(min(m(1), mpmath.sqrt(za)))
    sine = mpmath.cos(latS) / mpmath.sin(dist) * mpmath.sin(lon - lonS)
    azmsin = mpmath.asin(max(m(-1), min(m(1), sine)))
    cosine = (mpmath.sin(latS) - mpmath.sin(lat) * mpmath.cos(dist)) / (mpmath.cos(lat) * mpmath.sin(dist))
    azm = mpmath.acos(max(m(-1), min(m(1), cosine)))
    azm = -azm if azmsin > 0 else azm
    azm = azm - TWO_PI if azm >= PI else azm
    azm = azm + TWO_PI if azm < -PI else azm
    deg = azm * m(DEG)
    deg = deg - 360 * mpmath.floor(deg / 360)
    return deg, sine


def bt_exact(radiance: float, a: float, b: float):
    if not _finite(radiance, a, b):
        return math.nan
    R = max(m(radiance) * m(1e-2), m(1e-300))
    return m(b) / mpmath.log1p(m(a) / R)


def exact_array(fn, *arrays) -> np.ndarray:
    cols = [np.asarray(x).reshape(-1).tolist() for x in arrays]
    out = np.empty(len(cols[0]), dtype=object)
    for i, xs in enumerate(zip(*cols)):
        out[i] = fn(*xs)
    return out


def absolute_errors(got, exact, unit: float, circular: bool = False) -> np.ndarray:
    """|got - exact| / unit per element (``circular``: the distance on the circle of 360); inf where ``got`` is not finite."""
    out = np.empty(len(exact))
    for i, (g, x) in enumerate(zip(np.asarray(got, dtype=np.float64).reshape(-1).tolist(), exact.tolist())):
        if not math.isfinite(g):
            out[i] = math.inf
            continue
        d = abs(m(g) - x)
        if circular:
            d = d - 360 * mpmath.floor(d / 360)
            d = min(d, 360 - d)
        out[i] = float(d / unit)
    return out


# ---- the shared generators ----------------------------------------------------------------------------------------------------------
N_CASES, SEED = 3000, 0
_CACHE: dict = {}


def random_dates(rng, n: int) -> np.ndarray:
    """int64 nanoseconds between 1950 and 2060, at whole and fractional seconds."""
    lo, hi = (int(np.datetime64(d, "s").astype(np.int64)) for d in ("1950-01-01", "2060-01-01"))
    return rng.integers(lo, hi, n) * NS_SECOND + rng.integers(0, NS_SECOND, n) * (rng.random(n) < 0.5)


def forcing_cases(n: int = N_CASES, seed: int = SEED) -> dict:
    """date (int64 ns), latitude in +-90, longitude in [-180, 360]: julian day in [0, 366), hours in [0, 24)."""
    rng = np.random.default_rng(seed)
    return {"date": random_dates(rng, n), "latitude": rng.uniform(-90.0, 90.0, n), "longitude": rng.uniform(-180.0, 360.0, n)}


def view_cases(n: int = N_CASES, seed: int = SEED) -> dict:
    """Well-conditioned viewing geometry: sub-satellite longitudes from {0, 41.5, 45.5, -3.4} at latitude 0, observations within
    +-70 degrees of latitude and at least 2 from the satellite's, longitudes 2 to 65 degrees away on either side."""
    rng = np.random.default_rng(seed + 1)
    satlon = rng.choice([0.0, 41.5, 45.5, -3.4], n)
    lat = rng.uniform(2.0, 70.0, n) * rng.choice([-1.0, 1.0], n)
    lon = satlon + rng.uniform(2.0, 65.0, n) * rng.choice([-1.0, 1.0], n)
    return {"latitude": lat, "longitude": lon, "sat_latitude": np.zeros(n), "sat_longitude": satlon}


def bt_cases(n: int = N_CASES, seed: int = SEED) -> dict:
    """Channels of every band of both CrIS modes, radiances in [1e-3, 10^2.5] mW units; ``a``, ``b`` per case."""
    rng = np.random.default_rng(seed + 2)
    mode = rng.choice(["cris_fsr", "cris_nsr"], n)
    band = rng.integers(0, 3, n)
    channel = np.array([rng.integers(BANDS[md][bd][0], BANDS[md][bd][1] + 1) for md, bd in zip(mode, band)])
    a, b = np.empty(n), np.empty(n)
    for md in BANDS:
        a[mode == md], b[mode == md] = planck_tables(channel[mode == md], md)
    return {"radiance": 10.0 ** rng.uniform(-3.0, 2.5, n), "a": a, "b": b}


def composed(name: str) -> dict:
    """For ``name`` in cos_sza / azimuth / zenith / brightness_temperature on its generator: ``inputs``, ``exact`` (object array),
    ``numpy`` (the restatement's values), ``unit``, ``circular`` and ``skip`` (the rows the issue lets the ulp comparison leave out).
    Built once per process."""
    if name in _CACHE:
        return _CACHE[name]
    if name == "cos_sza":
        ins = forcing_cases()
        jd, hours = julian_day_and_hours(ins["date"])
        exact = exact_array(cos_sza_exact, jd, hours, ins["latitude"], ins["longitude"])
        value = cos_solar_zenith_angle(jd, hours, ins["latitude"], ins["longitude"])
        skip = np.array([abs(x) < 1e-14 for x in exact.tolist()])
        unclipped = exact
        exact = np.array([m(0) if x < 0 else x for x in exact.tolist()], dtype=object)  # the clip
        rec = dict(inputs=ins, exact=exact, numpy=value, unit=U53, circular=False, skip=skip, unclipped=unclipped)
    elif name in ("azimuth", "zenith"):
        ins = view_cases()
        cols = (ins["latitude"], ins["longitude"], ins["sat_latitude"], ins["sat_longitude"])
        if name == "azimuth":
            both = exact_array(azimuth_exact, *cols)
            exact = np.array([x[0] for x in both.tolist()], dtype=object)
            skip = np.array([abs(x[1]) < 1e-12 for x in both.tolist()])
            value = calc_azimuth(*cols)
        else:
            exact, skip, value = exact_array(zenith_exact, *cols), np.zeros(len(cols[0]), dtype=bool), calc_zenith(*cols)
        rec = dict(inputs=ins, exact=exact, numpy=value, unit=ULP360, circular=name == "azimuth", skip=skip)
    else:
        assert name == "brightness_temperature", name
        ins = bt_cases()
        exact = exact_array(bt_exact, ins["radiance"], ins["a"], ins["b"])
        rec = dict(inputs=ins, exact=exact, numpy=brightness_temperature(ins["radiance"], ins["a"], ins["b"]), unit=None, circular=False,
                   skip=np.zeros(len(exact), dtype=bool))
    _CACHE[name] = rec
    return rec


def errors(name: str, got, rows=None) -> np.ndarray:
    """The errors of ``got`` (values for the generator's rows ``rows``, all by default) in the statement's unit, skipped rows as 0."""
    rec = composed(name)
    rows = np.arange(len(rec["exact"])) if rows is None else np.asarray(rows)
    exact = rec["exact"][rows]
    if rec["unit"] is None:
        err = ulp_errors(np.asarray(got), exact, np.float64)
    else:
        err = absolute_errors(got, exact, rec["unit"], rec["circular"])
    return np.where(rec["skip"][rows], 0.0, err)


def single_forcing_exact(column: str, arguments: dict) -> np.ndarray:
    fn, variable = column.split("_", maxsplit=1)
    return exact_array(cos_exact if fn == "cos" else sin_exact, arguments[variable])


# ---- the seeded tables of the fixture -------------------------------------------------------------------------------------------
def _dates(*texts) -> np.ndarray:
    return np.array(texts, dtype="datetime64[ns]")


def forcings_table(seed: int = 4100, n: int = 48) -> dict:
    """NaT and NaN rows, dates before 1970, on 29 February, at 23:59:59.999999999 and at midnight on 1 January, longitudes on both
    sides of [0, 180]."""
    rng = np.random.default_rng(seed)
    date = random_dates(rng, n).view("datetime64[ns]")
    special = _dates("1969-12-31T23:59:59.999999999", "1961-03-04T05:06:07.5", "1900-02-28T12:00", "2024-02-29T00:00", "2024-02-29T23:59:59.999999999",
                     "2000-02-29T13:14:15", "2023-12-31T23:59:59.999999999", "2024-12-31T23:59:59.999999999", "2025-01-01T00:00", "2000-01-01T00:00",
                     "1970-01-01T00:00", "1969-01-01T00:00", "2025-04-01T06:00", "NaT", "NaT")
    date[: len(special)] = special
    lat, lon = rng.uniform(-90.0, 90.0, n), rng.uniform(-180.0, 360.0, n)
    lon[20:24] = [-179.5, -0.25, 180.25, 359.75]
    lat[24:28] = [-90.0, 90.0, 0.0, -0.0]
    lon[28:31] = [0.0, 180.0, 360.0]
    lat[31], lon[32], lat[33], lon[33] = np.nan, np.nan, np.nan, np.nan
    return {"date": date, "latitude": lat, "longitude": lon, "obsvalue": rng.standard_normal(n)}


def msg_table(seed: int, float_ids: bool, n: int = 64) -> dict:
    """Satellite ids on both sides of each of the four date thresholds (and exactly on them), unknown ids, NaT / NaN rows, rows that
    fail the azimuth mask in latitude only, in longitude only and in both; integer or float64 ids.  Every other row is as well
    conditioned as ``view_cases``: 2 to 70 degrees of latitude, 2 to 65 degrees of longitude from the sub-satellite point."""
    rng = np.random.default_rng(seed)
    ids = rng.choice([55, 56, 57, 70, 54, 71, 0], n)
    limit = np.array([np.datetime64(THRESHOLDS.get(int(s), ("2018-06-01",))[0], "ns").astype(np.int64) for s in ids])
    side = rng.choice([-1, 0, 1], n, p=[0.45, 0.1, 0.45])
    ns = limit + side * rng.integers(1, 400 * NS_DAY, n)
    ns[17:19] = NAT
    sat = ids.astype(np.float64) if float_ids else ids.astype(np.int64)
    if float_ids:
        sat[19:21] = np.nan
    satlon = meteosat_loc(sat, ns)[1].astype(np.float64)
    lat = rng.uniform(2.0, 70.0, n) * rng.choice([-1.0, 1.0], n)
    lon = satlon + rng.uniform(2.0, 65.0, n) * rng.choice([-1.0, 1.0], n)
    lat[0:5] = [0.0, 5e-6, -9e-6, 0.0, -0.0]  # latitude fails
    lon[5:9] = satlon[5:9] + [0.0, 5e-6, -9e-6, 0.0]  # longitude fails
    lat[9:12], lon[9:12] = 0.0, satlon[9:12]  # both fail
    lat[15], lon[16] = np.nan, np.nan
    return {"latitude": lat, "longitude": lon, "satellite_id": sat, "date": ns.view("datetime64[ns]")}


def azimuth_table(seed: int = 4300, n: int = 48) -> dict:
    """Per-row spacecraft positions at least 2 degrees from the observation in latitude and 2 to 65 in longitude, and rows that fail
    the mask in latitude only, in longitude only and in both; NaN rows."""
    rng = np.random.default_rng(seed)
    lat = rng.uniform(2.0, 70.0, n) * rng.choice([-1.0, 1.0], n)
    lon = rng.uniform(-180.0, 360.0, n)
    sc_lat = np.clip(lat + rng.uniform(2.0, 25.0, n) * rng.choice([-1.0, 1.0], n), -85.0, 85.0)
    sc_lon = lon + rng.uniform(2.0, 65.0, n) * rng.choice([-1.0, 1.0], n)
    sc_lat[0:3] = lat[0:3] + [0.0, 9e-6, -5e-6]  # latitude fails the mask
    sc_lon[3:6] = lon[3:6] + [0.0, 9e-6, -5e-6]  # longitude fails
    sc_lat[6:8], sc_lon[6:8] = lat[6:8], lon[6:8]  # both
    lat[8], sc_lon[9] = np.nan, np.nan
    return {"latitude": lat, "longitude": lon, "sc_lat": sc_lat, "sc_lon": sc_lon, "obsvalue": rng.standard_normal(n)}


def radiance_table(mode: str, seed: int, n: int = 8) -> dict:
    """Channels at every band edge of ``mode`` and outside all bands, in shuffled column order; radiances of 0, negative, 1e-310, NaN."""
    rng = np.random.default_rng(seed)
    edges = sorted({e for first, last, _, _ in BANDS[mode] for e in (first, last)} | {0, BANDS[mode][-1][1] + 1, 5000})
    channels = [int(c) for c in rng.permutation(edges + [7, 1000])]
    table = {"latitude": rng.uniform(-90.0, 90.0, n)}
    for j, ch in enumerate(channels):
        col = 10.0 ** rng.uniform(-3.0, 2.5, n)
        col[(j + np.arange(5)) % n] = [0.0, -1.5, 1e-310, np.nan, -0.0]
        table[f"obsvalue_rad_{ch}"] = col
        if j == 3:
            table["other"] = rng.standard_normal(n)
    return table


def seeded_cases() -> list[tuple[str, str, dict, dict]]:
    """``(id, filter, config, table)`` of every seeded table of the fixture."""
    return [
        ("seeded_forcings_all", "add_forcings", {"columns": ["cos_sza", "sin_longitude", "cos_julian_day", "sin_julian_day", "cos_local_time",
                                                             "sin_local_time", "cos_latitude", "sin_latitude", "cos_longitude"]}, forcings_table()),
        ("seeded_msg_integer_ids", "add_msg_angles", {"angle": "both"}, msg_table(4200, False)),
        ("seeded_msg_float_ids", "add_msg_angles", {"angle": "both", "azimuth": "az", "zenith": "zen"}, msg_table(4201, True)),
        ("seeded_azimuth", "add_azimuth", {"azimuth": "az", "spacecraft_latitude": "sc_lat", "spacecraft_longitude": "sc_lon"}, azimuth_table()),
        ("seeded_radiance_fsr", "radiance_to_brightness_temperature", {"mode": "cris_fsr"}, radiance_table("cris_fsr", 4400)),
        ("seeded_radiance_nsr", "radiance_to_brightness_temperature", {"mode": "cris_nsr", "output_prefix": "bt_"}, radiance_table("cris_nsr", 4401)),
    ]


# ---- the golden file ----------------------------------------------------------------------------------------------------------------
def load_golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


def golden_table(case: dict) -> dict:
    return {name: decode_column(spec) for name, spec in case["table"].items()}


def golden_expected(case: dict) -> dict:
    """The recorded frame in its column order: the fixture stores the columns the filter added or rewrote, the others are the table's."""
    table = golden_table(case)
    return {name: decode_column(case["expected"][name]) if name in case["expected"] else table[name] for name in case["columns"]}


# which added / rewritten columns must equal the recorded values bit for bit wherever they are NaN or 0.0 (specials and masks), and which
# statement's ceiling holds the rest
def statement_of(filter_name: str, config: dict, column: str) -> str | None:
    """The statement behind an output column: a name of ``CEILING``, "single" for a single-function forcing, None for a column the
    filter passes through."""
    if filter_name == "add_forcings":
        return None if column not in config["columns"] else ("cos_sza" if column == "cos_sza" else "single")
    if filter_name == "add_azimuth":
        return "azimuth" if column == config.get("azimuth", "azimuth") else None
    if filter_name == "add_msg_angles":
        angle = config.get("angle", "both")
        if angle in ("azimuth", "both") and column == config.get("azimuth", "azimuth"):
            return "azimuth"
        if angle in ("zenith", "both") and column == config.get("zenith", "zenith"):
            return "zenith"
        return None
    return "brightness_temperature" if column.startswith(config.get("output_prefix", "obsvalue_rawbt_")) else None
