"""Tables of observations: where they enter the field path, and the per-row columns recipes derive on the way (R: filters/tabular/).

``superob`` thins a raw table to one row per grid cell, time slot and report type (per-group means by pandas' rule:
``obs.group_means`` -> ``atx_obs_group_mean``); ``assign_to_grid`` adds the nearest grid point of every observation to the table;
``irregular_to_grid`` turns the table into one gridded field per target time and column, NaN where nothing was observed.  The fields it returns are levels of ONE stack in
HBM (``obs.grid_observations``: ``atx_obs_best_per_cell`` + ``atx_obs_fill_stack``), so a following ``regrid`` or per-point
filter finds them resident.

Between those steps recipes add per-row derived columns: ``add_forcings`` (solar and calendar forcings, ``obs.forcings`` ->
``atx_obs_forcings``), ``add_azimuth`` and ``add_msg_angles`` (satellite viewing geometry, ``obs.view_angles`` ->
``atx_obs_view_angles``) and ``radiance_to_brightness_temperature`` (the inverse Planck law for CrIS, ``obs.brightness_temperature`` ->
``atx_obs_planck_bt``) and ``add_healpix`` (the NESTED HEALPix pixel of every row, ``healpix.ang2pix`` -> ``atx_healpix_ang2pix``).  Each is
arithmetic over every row — one launch over columns that stay in HBM, so a chain such as
``superob | add_forcings | add_healpix | irregular_to_grid`` keeps a table of device tensors resident from raw rows to the stack.

The station-height pair sits there too: ``fill_orography`` replaces missing station altitudes (NaN or 9999.0) by the height of the
nearest point of a high-resolution orography — two searches and one gather per such row, ``obs.fill_heights`` ->
``atx_obs_fill_heights``, the orography resident in HBM per filter instance — and ``geopotential_to_height_tabular`` divides a column
by 9.80665 (numpy for host columns, torch true division for device tensors: one IEEE division either way, no kernel).

``apply_column_transformations`` evaluates ``log``, ``log1p``, ``safe_log``, ``sqrt``, ``exp``, ``abs``, ``sin``, ``sin_deg``, ``cos`` and
``cos_deg`` over whole columns, in config order and chained: up to 16 of them are one launch (``obs.column_ops`` ->
``atx_obs_column_ops``), and a transformation that reads an earlier one's target takes it from a register.

The row-set filters keep such a chain resident where it reorders or thins the table: ``sort_by`` (a stable multi-key sort by pandas'
order: ``obs.sort_order`` -> ``atx_obs_order_key`` and the library's stable radix sort), ``drop_duplicates`` (the first row of every
group of equal key tuples: ``obs.first_rows`` -> ``atx_obs_mark_first``) — both end in ONE gather of every column
(``obs.take_rows`` -> ``atx_obs_take_rows``) — and ``drop`` (columns leave; host bookkeeping, nothing is copied).

The QC filters mask, clip, fill and drop rows where recipes do it between those steps: ``mask_tabular``, ``mask_outside_range``,
``mask_infs``, ``mask_dewpoint_temperature``, ``exclude_dates``, ``remove_extreme_values``, ``clip_tabular``, ``impute_nans_tabular`` and
``drop_nans_tabular``.  Each compiles its configuration and the column dtypes into a program of compares and selects per row
(``obs.compile_*`` -> ``obs.row_program`` / ``obs.keep_rows`` -> ``atx_obs_column_ops``' second family of codes, up to 16 slots a launch); the
row-dropping ones end in one gather of every column (``Table.take``).  What comes back is pandas' to the bit and to the dtype: a float32
column is compared in float32 and stays float32, an integer column turns float64 only where a row was masked.

``filter_query`` and ``mask_values_custom`` take pandas' query language (``query``: the parser, numpy's typing, the postfix compiler): the
expression is one launch of the row-expression kernel (``obs.compile_query`` -> ``obs.query_rows`` / ``obs.eval_rows`` -> ``native.obs_row_expr``,
``native.obs_keep_positions``), a row filter writes a bit per row and ends in the same gather.

A table is a pandas DataFrame or a plain mapping ``name -> 1-D array / device tensor``.  Every ``forward`` wraps it in
``tables.Table``, which is where the table rule lives: which columns there are, where the launch runs, which columns are datetimes
and what goes back to the caller — a DataFrame for a DataFrame, a new dict of device tensors if any column was a tensor, else of
numpy arrays, never the caller's object (``with_columns``, ``replaced``, ``without``, ``take``).

Deviations from the reference, each said once when it first matters (``core.say_once``):
  * rows are taken by POSITION.  The reference goes through index labels (``df.loc[idxmin]``): a table whose index has duplicate
    labels would duplicate rows there.
  * ``spatial_index`` must be an integer column, or a float column whose non-missing entries are whole numbers; missing entries
    are dropped, as ``groupby`` drops them.
  * value columns must be numeric: they are read as float64, as the reference's float64 grids read them.  The per-row filters read
    latitude, longitude, spacecraft position and radiance columns as float64 as well (the reference would compute a float32 column
    in float32).
  * ``"h<nside>"`` grid names raise ``NotImplementedError``: the grid itself is ``healpix.grid(nside)``; the names are not wired to it yet.
  * ``superob``: the caller's table is not modified, and rows of equal ``date`` keep the first-appearance order of their groups.
  * ``add_azimuth``: the caller's table is not modified (the reference writes the new column into its argument).
  * ``add_healpix``: the caller's table is not modified either; healpy's ``ang2pix`` is restated, not called (``healpix`` module: equal
    away from pixel edges, where the last bit of cos / sin decides), and a row without a pixel (NaN or out-of-range latitude, non-finite
    longitude) raises ``ValueError``.
  * ``fill_orography``: the caller's table is not modified; the columns are read as float64 and the filled column is float64; the
    orography's axes must be 1-D, finite, non-empty and free of repeated values (the reference's answer on a repeated value is
    arbitrary); rows with two equally near axis entries are answered by the host's cKDTree, so every row is the reference's.
  * ``geopotential_to_height_tabular``: the caller's table is not modified; the column is read as float64.
  * ``apply_column_transformations``: float32 and float16 columns are read as float64 and the result is float64 (numpy would stay in
    float32); a ``source_column`` list of more than one name raises ``NotImplementedError``; numpy's ``RuntimeWarning``s are not
    reproduced.
  * ``sort_by``: a key column that cannot be ordered raises ``ValueError`` (the reference logs the error and returns the frame
    UNSORTED); an int64 device tensor named ``date`` is nanoseconds with NaT, as everywhere in this module.
  * ``sort_by`` / ``drop_duplicates``: a uint64 key column raises ``ValueError`` (it has no int64 key); the caller's table is not modified.
  * the QC filters: the caller's table is not modified; columns are read as float64 (exact for float32 and for integers below 2^53,
    beyond which nothing is specially handled); a bool column raises ``ValueError``; ``mask_outside_range`` with ``[None, None]`` leaves
    the column as it is (the reference raises) and raises ``ValueError`` for a missing column (the reference: ``KeyError``);
    ``impute_nans_tabular`` cannot fill a datetime or string column of a mapping (``ValueError``; a DataFrame's goes through pandas).
  * ``filter_query`` / ``mask_values_custom``: what pandas takes beyond the language of ``query`` (``@local``, ``//``, ``%``, ``**``, other
    functions, arithmetic or compares on booleans, datetimes) raises the reference's ``ValueError``; integers ride in float64 and never
    wrap; the caller's table is not modified.
  * ``encode_statids``: the caller's table is not modified; an entry that is not a ``str`` raises ``ValueError`` (the reference:
    ``AttributeError``); a trailing U+0000 is ignored; a value of 2^63 or more raises ``OverflowError`` for a mapping.

``encode_statids`` turns the one string column recipes carry, the station identifier, into int64 (``obs.encode_statids`` ->
``atx_text_encode_statids`` of the companion library ``libatx_text``, one launch over the column's byte matrix), after which the whole
table is numeric and resident; ``rename_tabular`` renames columns (host bookkeeping).  With them every tabular filter of the reference
is registered here.
"""

from __future__ import annotations

import datetime
import logging
from typing import Any

import numpy as np
import torch

from .. import healpix, obs, query
from ..core import Filter, filter_registry, say_once
from ..fields import MISSING, Field, FieldList, new_field_from_stack
from ..grids import lookup
from ..tables import NAT, Table, column_kind, dtype_kind, float_column, host_array, on_device, text_matrix, to_ns

LOG = logging.getLogger(__name__)


def _healpix(grid: str) -> bool:
    return isinstance(grid, str) and grid[:1] == "h" and grid[1:].isdigit()


def _named_grid(grid: str) -> tuple[np.ndarray, np.ndarray]:
    """``(latitudes, longitudes)`` of a named grid, longitudes above 180 wrapped by -360 (R: support/superob.py:19-25)."""
    if _healpix(grid):
        raise NotImplementedError(f"grid {grid!r}: HEALPix grids need healpy, which this package does not use; "
                                  "octahedral / full Gaussian names, lat-lon increments and .npz files are available")
    info = lookup(grid)
    lon = np.where(info["longitudes"] > 180, info["longitudes"] - 360, info["longitudes"])
    return info["latitudes"], lon


class _GridTemplate(Field):
    """What the fields of one ``irregular_to_grid`` call share: the grid.  It carries no metadata and no data of its own."""

    def __init__(self, latitudes: np.ndarray, longitudes: np.ndarray) -> None:
        self._latitudes = np.asarray(latitudes)
        self._longitudes = np.asarray(longitudes)
        self.shape = (len(self._latitudes),)

    def _flat(self) -> np.ndarray:
        raise NotImplementedError("the grid template of irregular_to_grid holds no values")

    def grid_points(self) -> tuple[np.ndarray, np.ndarray]:
        return self._latitudes, self._longitudes

    def _lookup(self, key: str) -> Any:
        if key == "latitudes":
            return self._latitudes
        if key == "longitudes":
            return self._longitudes
        return MISSING

    def _metadata_keys(self) -> list[str]:
        return ["param", "valid_datetime", "latitudes", "longitudes"]  # the keys of the reference's list-of-dicts entries

    def __repr__(self) -> str:
        return f"ObservationGrid({self.shape[0]} points)"


def _to_datetime(ns: int) -> datetime.datetime | None:
    """``pd.Timestamp(ns).to_pydatetime()``: microseconds kept, the nanoseconds below them dropped; NaT -> None."""
    if ns == NAT:
        return None
    return datetime.datetime(1970, 1, 1) + datetime.timedelta(microseconds=int(ns) // 1000)


class IrregularToGrid(Filter):
    """Irregular observations within a time window to gridded fields (R: filters/tabular/irregular_to_grid.py:25-161).

    For every distinct value of ``window_date_column`` (in order of first appearance) and every name in ``columns``, one field
    on the named ``grid``: at each grid point the value of the best observation whose ``spatial_index`` is that point and whose
    ``date`` lies in ``window`` around the target (default ``"(-time_freq, 0]"``), NaN where there is none.  Best is the smallest
    ``|date - target| / time_freq``; with ``nan_score_weight`` w > 0 the smallest
    ``(1 - w) * that + w * nan_count / len(columns)``; among equals the first row of the table.  Rows whose ``columns`` are all
    NaN never take part; spatial indices outside the grid are ignored.

    The input needs the columns ``date``, ``spatial_index``, ``window_date_column`` and ``columns``; it is a DataFrame or a
    mapping of 1-D arrays / device tensors (dates as datetime64 or int64 nanoseconds).  The output is this package's
    ``FieldList``, time-major then by column; every field is a level of one float64 stack in HBM and carries ``param`` (the
    column name) and ``valid_datetime`` (the target).

    Deviations: rows are taken by position (a DataFrame's index labels are not consulted); ``spatial_index`` must be an integer
    column or a float column of whole numbers (missing entries are dropped); value columns must be numeric.
    """

    def __init__(self, window_date_column: str, columns: list[str], time_freq: str = "6h", grid: str = "o96",
                 window: str | None = None, nan_score_weight: float = 0.0) -> None:
        self.window_date_column = window_date_column
        self.columns = columns
        self.time_freq = time_freq
        self.grid = grid
        if not self.columns:
            raise ValueError("At least one column must be specified")
        if not self.window_date_column:
            raise ValueError("window_date_column must be specified")
        self.freq_ns = obs.parse_frequency(time_freq)
        self.window = obs.parse_window(window or f"(-{time_freq}, 0]")
        if not (0.0 <= nan_score_weight <= 1.0):
            raise ValueError("nan_score_weight must be in the range [0.0, 1.0]")
        self.nan_score_weight = nan_score_weight
        say_once(LOG, (type(self), "deviations"), "irregular_to_grid: rows are taken by position (index labels are not consulted), "
                 "spatial_index must hold whole numbers (missing entries are dropped) and value columns are read as float64",
                 level=logging.INFO)

    def __repr__(self) -> str:
        return f"IrregularToGrid({list(self.columns)}, grid={self.grid!r})"

    @staticmethod
    def _define_grid(grid: str) -> tuple[np.ndarray, np.ndarray]:
        """R: irregular_to_grid.py:319-325 — static and patchable, as the reference's tests patch it."""
        return _named_grid(grid)

    def forward(self, table: Any) -> FieldList:
        t = Table(table)
        t.require(["date", "spatial_index", self.window_date_column] + list(self.columns))
        if t.frame and not table.index.is_unique:
            say_once(LOG, (type(self), "position"), "irregular_to_grid: the table's index has duplicate labels; rows are taken by "
                     "position here, the reference would repeat the rows of a duplicated label")
        cells = t["spatial_index"]
        if column_kind(cells) == "f":
            say_once(LOG, (type(self), "float-index"), "irregular_to_grid: spatial_index is a float column; whole numbers are "
                     "read as indices and missing entries dropped", level=logging.INFO)
        latitudes, longitudes = self._define_grid(self.grid)
        window_ns = to_ns(t[self.window_date_column])
        targets = obs.unique_in_order(window_ns)
        stack = obs.grid_observations(t["date"], cells, [t[c] for c in self.columns], targets, n_cells=len(latitudes),
                                      window=self.window, freq=self.freq_ns, weight=self.nan_score_weight)
        template = _GridTemplate(latitudes, longitudes)
        fields = []
        for t, target in enumerate(targets):
            valid = _to_datetime(int(target))
            for c, param in enumerate(self.columns):
                fields.append(new_field_from_stack(stack, t * len(self.columns) + c, template=template,
                                                   metadata=dict(param=param, valid_datetime=valid)))
        return FieldList(fields)


class AssignToGrid(Filter):
    """Adds ``grid_index_{grid}`` (the nearest grid point of every row's ``latitude`` / ``longitude``) and ``distance`` to the table
    (R: filters/tabular/assign_to_grid.py:18-63).

    Nearest in the PLANE of (latitude, longitude) degrees, with the grid's longitudes wrapped to (-180, 180] — the reference's
    ``cKDTree(column_stack([lat, lon]))``, not the sphere: an observation at longitude 359.9 is 179.9 degrees from everything,
    as the reference's test pins.  Searched on the device (``obs.nearest_grid_index``); indices and distances are cKDTree's bit
    for bit.  Returns the kind of table it was given: ``DataFrame.assign`` for a DataFrame, a new dict for a mapping."""

    def __init__(self, *, grid: str) -> None:
        if not grid:
            raise ValueError("No grid specified.")
        self.grid = grid

    def __repr__(self) -> str:
        return f"AssignToGrid(grid={self.grid!r})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        t.require(["latitude", "longitude"])
        grid_lat, grid_lon = _named_grid(self.grid)
        distances, indices = obs.nearest_grid_index(grid_lat, grid_lon, t["latitude"], t["longitude"])  # host arrays: the search's own crossing
        added = {f"grid_index_{self.grid}": indices, "distance": distances}
        return table.assign(**added) if t.frame else {**table, **added}


class SuperOb(Filter):
    """One row per grid cell, time slot and report type (R: filters/tabular/superob.py:21-97, support/superob.py:43-69).

    Rows without ``date``, ``latitude`` or ``longitude`` are dropped.  Every remaining row gets ``spatial_index`` and ``distance``
    (its nearest point of ``grid`` in the plane of (latitude, longitude) degrees, as ``assign_to_grid``), a time slot
    ``(date - min(date)) // timeslot_length`` and ``grid_index = spatial_index + n_grid * slot``.  The rows are grouped by
    ``(grid_index, *columns_to_groupby)``, groups in order of first appearance, rows with a missing key entry dropped.  Per group,
    every column that is neither a key nor in ``columns_to_take_nearest`` gets its MEAN BY PANDAS' RULE — one Kahan sum in the row
    order of the table, missing values skipped (``obs.group_means`` -> ``atx_obs_group_mean``; bit-equal to
    ``groupby(sort=False).mean()``, float64 out, ``date`` stays a datetime) — and every column in ``columns_to_take_nearest`` the value of the
    row of smallest ``distance``, the first such row among equals (``atx_obs_group_argmin``).  ``grid_index`` and ``distance`` are
    dropped; columns come as ``columns_to_groupby``, the averaged columns in table order, ``columns_to_take_nearest``; rows are
    sorted by ``date``.

    ``grid="native"`` and an empty table are returned as given.  The result is the kind of table that came in: a DataFrame for a
    DataFrame; for a mapping a dict of device tensors (dates as int64 nanoseconds) if any input column was a device tensor,
    else of numpy arrays — so ``superob | irregular_to_grid`` can keep a table resident from raw rows to the stack.

    Deviations: rows are taken by position (index labels are not consulted); the caller's DataFrame is NOT modified (the
    reference's ``dropna(inplace=True)`` modifies it); rows of equal ``date`` keep the first-appearance order of their groups (a
    stable sort; pandas' default quicksort leaves them in an order that depends on numpy's build); ``"h<nside>"`` grids need healpy
    and raise ``NotImplementedError``.
    """

    def __init__(self, *, grid: str, timeslot_length: int, columns_to_take_nearest: list[str] | None = None,
                 columns_to_groupby: list[str] | None = None) -> None:
        if not isinstance(grid, str) or not grid:
            raise ValueError("No grid specified.")
        seconds = timeslot_length
        if isinstance(seconds, bool) or not isinstance(seconds, (int, float, np.integer, np.floating)) or seconds != seconds \
                or seconds <= 0 or seconds != int(seconds):
            raise ValueError(f"timeslot_length must be a positive whole number of seconds, got {timeslot_length!r}")
        self.grid = grid
        self.timeslot_length = int(seconds)
        self.columns_to_take_nearest = list(columns_to_take_nearest) if columns_to_take_nearest else []
        self.columns_to_groupby = list(columns_to_groupby) if columns_to_groupby else []
        both = set(self.columns_to_take_nearest) & (set(self.columns_to_groupby) | {"grid_index"})
        if both:
            raise ValueError(f"columns both grouped by and taken from the nearest row: {sorted(both)}")
        say_once(LOG, (type(self), "deviations"), "superob: rows are taken by position (index labels are not consulted), the caller's "
                 "table is not modified, and rows of equal date keep the first-appearance order of their groups (a stable sort)",
                 level=logging.INFO)

    def __repr__(self) -> str:
        return f"SuperOb(grid={self.grid!r}, timeslot_length={self.timeslot_length})"

    @staticmethod
    def _define_grid(grid: str) -> tuple[np.ndarray, np.ndarray]:
        """R: support/superob.py:19-25 — static and patchable, as ``IrregularToGrid._define_grid``."""
        return _named_grid(grid)

    def forward(self, table: Any) -> Any:
        t = Table(table)
        if self.grid == "native" or t.n_rows == 0:
            return table
        grid_lat, grid_lon = self._define_grid(self.grid)
        t.require(["date", "latitude", "longitude"] + self.columns_to_groupby + self.columns_to_take_nearest)
        if t.frame and not table.index.is_unique:
            say_once(LOG, (type(self), "position"), "superob: the table's index has duplicate labels; rows are taken by position "
                     "here, the reference would repeat the rows of a duplicated label")
        return _superob(self, t, grid_lat, grid_lon)


def _superob(f: SuperOb, t: Table, grid_lat: np.ndarray, grid_lon: np.ndarray) -> Any:
    dev = t.device
    # R: superob.py:72 — rows without date / latitude / longitude leave (here: a copy of the rest, the caller's table stays)
    gone = t.missing("date", dev) | t.missing("latitude", dev) | t.missing("longitude", dev)
    if bool(gone.any()):
        t = Table(t.take(torch.nonzero(~gone).reshape(-1)), like=t)
    n = t.n_rows
    if n == 0:
        return t.table
    # R: support/superob.py:43-69
    distance, spatial = obs.nearest_grid_index(grid_lat, grid_lon, t["latitude"], t["longitude"])
    distance, spatial = on_device(np.asarray(distance, dtype=np.float64), dev), on_device(np.asarray(spatial, dtype=np.int64), dev)
    date = on_device(to_ns(t["date"]), dev)
    slot = (date - date.min()) // (f.timeslot_length * 10**9)
    added = {"grid_index": spatial + len(grid_lat) * slot, "spatial_index": spatial, "distance": distance}
    names = list(dict.fromkeys(t.names + list(added)))  # DataFrame.assign: an existing column keeps its place, a new one goes to the end
    key_names = ["grid_index"] + f.columns_to_groupby
    averaged = [c for c in names if c not in set(key_names) | set(f.columns_to_take_nearest)]
    asked = {c: added[c] for c in f.columns_to_groupby + f.columns_to_take_nearest if c in added}
    if asked:  # the table came with a column of that name (superob's own output does): the new one replaces it before rows are taken
        t = Table(t.with_columns(asked), like=t)
    # R: superob.py:86-88
    keys, valid = [], None
    for name in key_names:
        codes, ok = obs.key_codes(added[name] if name in added else t[name])
        if ok is None and name not in added and t.is_datetime(name):  # int64 nanoseconds on the device: NaT is a missing key there too
            ok = codes != NAT
        keys.append(codes)
        if ok is not None:
            ok = on_device(ok, dev)
            valid = ok if valid is None else valid & ok
    groups = obs.superob_groups(keys, valid, dev)
    values = torch.empty((len(averaged), n), dtype=torch.float64, device=dev)
    for j, name in enumerate(averaged):
        if name in added:
            values[j].copy_(added[name])
        else:
            t.as_float64(name, values[j])
    mean, _ = obs.group_means(values, groups)
    nearest = obs.group_nearest(distance, groups)
    # R: superob.py:94-96 — groups in order of first appearance, then a stable sort by date (NaT last)
    mean_of = {name: mean[j] for j, name in enumerate(averaged)}

    def as_ns(m: torch.Tensor) -> torch.Tensor:
        # pandas: the float64 quotient truncated back to int64, NaT where nothing was summed
        return torch.where(torch.isnan(m), torch.zeros_like(m), m).to(torch.int64).masked_fill_(torch.isnan(m), NAT)

    when = as_ns(mean_of["date"]) if "date" in mean_of else date[groups.first if "date" in key_names else nearest]
    when = when[groups.appearance]
    by_date = torch.argsort(torch.where(when == NAT, torch.full_like(when, torch.iinfo(torch.int64).max), when), stable=True)
    final = groups.appearance[by_date]
    # columns_to_groupby, the averaged columns in table order, columns_to_take_nearest: two row sets, one gather each
    dates = [name for name in averaged if name not in added and t.is_datetime(name)]
    means = {name: (as_ns(m[final]) if name in dates else m[final]) for name, m in mean_of.items() if name != "distance"}
    out = Table(t.take(groups.first[final], f.columns_to_groupby), like=t).with_columns(means, datetimes=dates)
    near = t.take(nearest[final], f.columns_to_take_nearest)
    if not t.frame:
        return {**out, **near}
    out = out.reset_index(drop=True).join(near.reset_index(drop=True))
    out.index = by_date.cpu().numpy()  # pandas keeps the group numbers through sort_values
    return out


# ---- per-row derived columns ---------------------------------------------------------------------------------------------------------
class AddForcings(Filter):
    """Adds solar and calendar forcing columns to the table (R: filters/tabular/add_forcings.py:19-127,
    support/compute_forcings.py:14-87).

    ``columns``: names from ``cos_julian_day``, ``sin_julian_day``, ``cos_sza``, ``sin_local_time``, ``cos_local_time``,
    ``cos_latitude``, ``sin_latitude``, ``cos_longitude``, ``sin_longitude``; anything else raises ``ValueError``.  The table needs
    ``date`` (datetime64 or int64 nanoseconds), ``latitude`` and ``longitude``.  The julian day counts WHOLE days and seconds from
    1 January of the date's year (``Timedelta.days`` / ``.seconds``); NaT gives NaN in every date-dependent column; ``cos_sza`` is
    clipped at 0.  One launch (``obs.forcings`` -> ``atx_obs_forcings``) whatever the number of columns.

    Deviation: latitude and longitude are read as float64."""

    SUPPORTED_FORCINGS = set(obs.FORCINGS)

    def __init__(self, *, columns: list[str]) -> None:
        if not set(columns).issubset(self.SUPPORTED_FORCINGS):
            raise ValueError(f"Unknown columns requested: {set(columns) - self.SUPPORTED_FORCINGS}")
        self.columns = columns

    def __repr__(self) -> str:
        return f"AddForcings({list(self.columns)})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        t.require(["date", "latitude", "longitude"])
        return t.with_columns(obs.forcings(t["date"], t["latitude"], t["longitude"], list(self.columns), dev=t.device))


class AddAzimuth(Filter):
    """Adds the viewing azimuth of a spacecraft whose position every row carries (R: filters/tabular/add_azimuth.py:19-62,
    support/sat_view_angles.py:52-97).  ``azimuth``, ``spacecraft_latitude`` and ``spacecraft_longitude`` name the columns; a missing
    spacecraft column raises ``ValueError``.  Exactly 0.0 where the spacecraft is within 0.00001 degrees in latitude OR longitude
    (a NaN included).  ``obs.view_angles`` -> ``atx_obs_view_angles``.

    Deviations: the caller's table is not modified (the reference writes the column into its argument); the four columns are read
    as float64."""

    def __init__(self, *, azimuth: str = "azimuth", spacecraft_latitude: str = "spacecraft_latitude",
                 spacecraft_longitude: str = "spacecraft_longitude") -> None:
        self.azimuth = azimuth
        self.spacecraft_latitude = spacecraft_latitude
        self.spacecraft_longitude = spacecraft_longitude
        say_once(LOG, (type(self), "deviations"), "add_azimuth: the caller's table is not modified (the reference writes the azimuth "
                 "column into its argument), and the position columns are read as float64", level=logging.INFO)

    def __repr__(self) -> str:
        return f"AddAzimuth({self.azimuth!r})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        t.require([self.spacecraft_latitude, self.spacecraft_longitude])
        t.require(["latitude", "longitude"])
        angles = obs.view_angles(t["latitude"], t["longitude"], t[self.spacecraft_latitude], t[self.spacecraft_longitude],
                                 azimuth=True, zenith=False, dev=t.device)
        return t.with_columns({self.azimuth: angles["azimuth"]})


class AddMSGAngles(Filter):
    """Adds the Meteosat viewing azimuth and / or zenith (R: filters/tabular/add_msg_angles.py:22-81,
    support/sat_view_angles.py:17-132).  ``angle``: ``"azimuth"``, ``"zenith"`` or ``"both"`` (anything else: ``ValueError``);
    ``azimuth``, ``zenith`` and ``satellite_id`` name the columns; a table without the id column raises ``ValueError``.

    The sub-satellite point comes from the id and the date (``obs.meteosat_position``): latitude 0; longitude 41.5 for id 55 after
    2016-10-20, 45.5 for 56 after 2022-05-08, -3.4 for 57 before 2013-01-24 and for 70 before 2015-12-01 (strict comparisons), 0
    otherwise — stored IN THE DTYPE OF THE ID COLUMN, as the reference's ``np.zeros_like(satids)`` stores it: with integer ids, which
    the reference's own tests use, the longitudes are 41 / 45 / -3, and its expected literals depend on it.  The table is built with
    torch on the device; the angles are ``obs.view_angles`` -> ``atx_obs_view_angles``.

    Deviation: latitude, longitude and the sub-satellite table are read as float64 by the kernel (a float32 id column gives float32
    sub-satellite longitudes first, as the reference's does)."""

    def __init__(self, *, angle: str = "both", azimuth: str = "azimuth", zenith: str = "zenith", satellite_id: str = "satellite_id") -> None:
        if angle not in ("azimuth", "zenith", "both"):
            raise ValueError(f"Invalid angle: {angle}. Must be 'azimuth', 'zenith' or 'both'.")
        self.angle = ("azimuth", "zenith") if angle == "both" else (angle,)
        self.azimuth = azimuth
        self.zenith = zenith
        self.satellite_id = satellite_id

    def __repr__(self) -> str:
        return f"AddMSGAngles({'+'.join(self.angle)})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        if self.satellite_id not in t.names:
            raise ValueError(f"DataFrame must contain a column '{self.satellite_id}' for MSG angles calculation.")
        t.require(["latitude", "longitude", "date"])
        sat_lat, sat_lon = obs.meteosat_position(t[self.satellite_id], t["date"], dev=t.device)
        angles = obs.view_angles(t["latitude"], t["longitude"], sat_lat, sat_lon, azimuth="azimuth" in self.angle,
                                 zenith="zenith" in self.angle, dev=t.device)
        return t.with_columns({getattr(self, name): angles[name] for name in self.angle})


class RadianceToBrightnessTemperature(Filter):
    """CrIS NSR / FSR radiances in mW/(m^2 sr cm^-1) to brightness temperatures in K
    (R: filters/tabular/radiance_to_brightness_temperature.py:20-120).  Every column whose name starts with ``input_prefix`` and ends
    in ``_<channel number>`` is replaced, in place in the column order, by ``<output_prefix><channel number>``; no such column raises
    ``ValueError``, and so does a ``mode`` other than ``"cris_fsr"`` / ``"cris_nsr"``.  The columns are sorted by channel number and
    stacked into one ``[n_ch, n]`` block, converted in ONE launch (``obs.brightness_temperature`` -> ``atx_obs_planck_bt``) and handed
    back row by row.  A channel outside the bands of the mode has no wavenumber: its column comes back NaN.  Radiances of zero,
    negative or below 1e-298 are floored (``maximum(R * 1e-2, 1e-300)``).

    Deviation: radiance columns are read as float64."""

    def __init__(self, *, mode: str, input_prefix: str = "obsvalue_rad_", output_prefix: str = "obsvalue_rawbt_") -> None:
        if mode not in ("cris_fsr", "cris_nsr"):
            raise ValueError(f"Invalid mode: {mode}. Must be 'cris_fsr' or 'cris_nsr'.")
        self.mode = mode
        self.input_prefix = input_prefix
        self.output_prefix = output_prefix

    def __repr__(self) -> str:
        return f"RadianceToBrightnessTemperature({self.mode!r})"

    def forward(self, table: Any) -> Any:
        import re

        t = Table(table)
        cols = [c for c in t.names if isinstance(c, str) and c.startswith(self.input_prefix)]
        if not cols:
            raise ValueError(f"No columns starting with '{self.input_prefix}' found in DataFrame.")
        found = [re.search(r"_(\d+)$", c) for c in cols]
        if not all(found):
            raise ValueError(f"columns without a trailing channel number: {[c for c, m in zip(cols, found) if not m]}")
        # R: :89-94 — sorted by channel, so that wavenumbers and columns line up
        chans = np.array([int(m.group(1)) for m in found], dtype=np.int64)
        order = np.argsort(chans, kind="stable")
        cols, chans = [cols[i] for i in order], chans[order]
        radiance = torch.stack([float_column(t[c], t.device) for c in cols])
        tb = obs.brightness_temperature(radiance, obs.cris_wavenumbers(chans, self.mode), out=radiance)
        return t.replaced(dict(zip(cols, tb)), renamed={c: f"{self.output_prefix}{ch}" for c, ch in zip(cols, chans)})


class AddHealpix(Filter):
    """Adds ``healpix_idx_{nside}``, the NESTED HEALPix pixel of every row's ``longitude`` / ``latitude``, as the last column
    (R: filters/tabular/add_healpix.py:18-51: ``hp.ang2pix(nside, lon, lat, nest=True, lonlat=True)``).  ``nside <= 0`` raises
    ``ValueError`` at construction, as in the reference; an ``nside`` that is not a power of two raises it at ``forward``, where healpy's
    ``check_nside`` would.  int64, one launch (``healpix.ang2pix`` -> ``atx_healpix_ang2pix``); a table of device tensors stays one.

    Deviations: the caller's table is not modified (the reference writes the column into its argument); the two columns are read as
    float64; a NaN or out-of-range latitude or a non-finite longitude raises ``ValueError``; healpy is restated, not called — pinned by
    the reference's literals and equal to the exact geometry away from pixel edges (``healpix`` module)."""

    def __init__(self, *, nside: int = 32) -> None:
        if nside <= 0:
            raise ValueError("nside must be a positive integer.")
        self.nside = nside
        healpix.parity_note()
        say_once(LOG, (type(self), "table"), "add_healpix: the caller's table is not modified (the reference writes the index column "
                 "into its argument)", level=logging.INFO)
        say_once(LOG, (type(self), "float64"), "add_healpix: latitude and longitude are read as float64", level=logging.INFO)
        say_once(LOG, (type(self), "bad-rows"), "add_healpix: a NaN or out-of-range latitude or a non-finite longitude raises ValueError "
                 "(healpy's own check of theta is restated from memory and is not pinned by the reference's tests)", level=logging.INFO)

    def __repr__(self) -> str:
        return f"AddHealpix(nside={self.nside})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        t.require(["latitude", "longitude"])
        healpix.check_nside(self.nside, nest=True)
        index = healpix.ang2pix(self.nside, t["longitude"], t["latitude"], nest=True, dev=t.device)
        return t.with_columns({f"healpix_idx_{self.nside}": index})


class FillHeights(Filter):
    """Fills the missing station altitudes of a table from a high-resolution orography (R: filters/tabular/fill_heights.py:23-91,
    support/utils.py:24-55 ``get_heights``).  A row whose ``station_altitude`` is NaN or exactly 9999.0 gets ``heights[i, j]`` of the
    orography file, ``i`` / ``j`` the entries of the file's latitude / longitude axis nearest to the row's ``latitude`` /
    ``longitude`` as ``cKDTree(np.c_[axis]).query`` decides it — per axis, in degrees, WITHOUT wrap-around in longitude (359.9 against
    an axis 0 .. 359 gives 359: the reference's behaviour, kept), the end of an axis for a row beyond it.  Every other row keeps its
    bits.  One launch over columns that stay in HBM (``obs.fill_heights`` -> ``atx_obs_fill_heights``); rows with two equally near
    entries on an axis are answered by the host's cKDTree, so every row is the reference's.  A table without the altitude column
    raises ``ValueError``; a row to fill with a NaN or infinite coordinate raises it too (cKDTree refuses such a query).

    The file is opened once per instance, on first use (``_open_orography``); its axes are sorted and uploaded with the heights once
    (``obs.HeightGrid``).  Returns the kind of table it was given; a table of device tensors stays one.

    Deviations: the caller's table is not modified (the reference writes into its argument); the three columns are read as float64
    and the filled column is float64; both axes of the file must be 1-D, finite, non-empty and without repeated values, and the
    heights ``[n_lat, n_lon]`` (the reference's answer on a repeated axis value is arbitrary)."""

    def __init__(self, *, orography_file: str, station_altitude: str = "stalt", orography_altitude: str = "z",
                 orography_latitude: str = "latitude", orography_longitude: str = "longitude") -> None:
        self.orography_file = orography_file
        self.station_altitude = station_altitude
        self.orography_altitude = orography_altitude
        self.orography_latitude = orography_latitude
        self.orography_longitude = orography_longitude
        self._grid: obs.HeightGrid | None = None
        say_once(LOG, (type(self), "table"), "fill_orography: the caller's table is not modified (the reference writes the filled "
                 "altitudes into its argument)", level=logging.INFO)
        say_once(LOG, (type(self), "float64"), "fill_orography: latitude, longitude and the station altitude are read as float64, and "
                 "the filled column is float64", level=logging.INFO)
        say_once(LOG, (type(self), "axes"), "fill_orography: both orography axes must be 1-D, finite, non-empty and without repeated "
                 "values, and the heights [n_lat, n_lon]; anything else raises ValueError", level=logging.INFO)

    def __repr__(self) -> str:
        return f"FillHeights({self.station_altitude!r}, orography_file={self.orography_file!r})"

    @staticmethod
    def _open_orography(path: str, altitude: str, latitude: str, longitude: str) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(latitude axis, longitude axis, heights)`` of the file (R: fill_heights.py:74-77) — static and patchable, as
        ``IrregularToGrid._define_grid``.  An ``.npz`` holding the three named arrays is read with numpy; anything else goes to
        ``xarray.open_dataset`` when xarray can be imported."""
        if str(path).endswith(".npz"):
            with np.load(path) as data:
                missing = [name for name in (latitude, longitude, altitude) if name not in data.files]
                if missing:
                    raise ValueError(f"{path}: no arrays named {missing}; the file holds {list(data.files)}")
                return data[latitude], data[longitude], data[altitude]
        try:
            import xarray as xr
        except ImportError:
            raise ValueError(f"cannot read the orography {path!r}: give an .npz file holding the arrays {latitude!r}, {longitude!r} and "
                             f"{altitude!r}, or install xarray for everything xarray.open_dataset reads") from None
        ds = xr.open_dataset(path)
        return np.array(ds[latitude]), np.array(ds[longitude]), np.array(ds[altitude])

    def grid(self) -> obs.HeightGrid:
        """The orography in HBM: read, checked, sorted and uploaded on first use, then kept."""
        if self._grid is None:
            self._grid = obs.HeightGrid(*self._open_orography(self.orography_file, self.orography_altitude, self.orography_latitude,
                                                              self.orography_longitude))
        return self._grid

    def forward(self, table: Any) -> Any:
        t = Table(table)
        t.require([self.station_altitude])
        t.require(["latitude", "longitude"])
        grid = self.grid()  # the file's checks come before anything touches the device
        return t.with_columns({self.station_altitude: obs.fill_heights(grid, t["latitude"], t["longitude"], t[self.station_altitude])})


class GeopotentialToHeightTabular(Filter):
    """``table[height] = table[geopotential] / 9.80665`` (R: filters/tabular/geopotential_to_height.py:20-52); ``height`` defaults to
    the geopotential column, which is then replaced.  One IEEE division in float64: numpy for host columns, torch true division for
    device tensors — the same bits, so no kernel.  A table without the geopotential column raises ``ValueError``.

    Deviations: the caller's table is not modified; the column is read as float64."""

    G = 9.80665

    def __init__(self, *, geopotential: str, height: str | None = None) -> None:
        self.geopotential = geopotential
        self.height = height if height else geopotential
        say_once(LOG, (type(self), "deviations"), "geopotential_to_height_tabular: the caller's table is not modified (the reference "
                 "writes the height column into its argument), and the geopotential is read as float64", level=logging.INFO)

    def __repr__(self) -> str:
        return f"GeopotentialToHeightTabular({self.geopotential!r} -> {self.height!r})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        t.require([self.geopotential])
        z = t[self.geopotential]
        if t.frame:
            return table.assign(**{self.height: z.astype(np.float64) / self.G})
        if not t.resident:
            return {**table, self.height: np.asarray(host_array(z), dtype=np.float64) / self.G}
        # the divisor as a tensor on z's device: torch turns division by a Python number into a multiplication by its
        # reciprocal on the device, which is two roundings and not numpy's quotient
        z = float_column(z, t.device)
        return t.with_columns({self.height: torch.true_divide(z, torch.full((), self.G, dtype=torch.float64, device=z.device))})


def column_ops_parity_note() -> None:
    """Said once per process, by the first ``apply_column_transformations`` filter: what its values are held to."""
    say_once(LOG, "column-ops-parity", "apply_column_transformations: sqrt and abs have numpy's bits; log, log1p, safe_log and exp are "
             "held within 1 ulp of exact arithmetic, sin / cos (and sin_deg / cos_deg of numpy's own x * (pi / 180)) within 1 ulp for "
             "arguments below 1e5 and 2 ulps beyond — not to numpy's last bit, which is itself up to an ulp from exact")


class ApplyColumnTransformations(Filter):
    """Applies library functions to columns of a table (R: filters/tabular/apply_column_transformations.py:18-138).  ``**config`` maps a
    target column to ``{"function": name, "source_column": column}``; ``function`` is one of ``log``, ``log1p``, ``safe_log``
    (``log(x + 1e-10)``), ``sqrt``, ``exp``, ``abs``, ``sin``, ``sin_deg``, ``cos``, ``cos_deg``; ``source_column`` defaults to the target,
    which is then replaced.  An empty config, a specification that is not a dict or has no ``function``, and an unknown function raise
    ``ValueError`` at construction; a source column the table lacks raises ``KeyError`` at ``forward``.

    Transformations apply in config order, so a later one sees an earlier one's result.  Up to 16 of them run as ONE launch
    (``obs.column_ops`` -> ``atx_obs_column_ops``), a chained one taking its operand from a register.  float64 and integer columns give
    what numpy gives: float64 — and ``abs`` of an integer column keeps its dtype (``torch.abs``, outside the kernel).  A bool or
    non-numeric source raises ``ValueError``.  A DataFrame gives a DataFrame with existing columns in place and new ones appended in
    config order (``assign``); a mapping gives a new dict, of device tensors if any input column was one, else of numpy arrays.  The
    caller's table is untouched.

    Deviations: float32 and float16 columns are read as float64 and the result is float64 (numpy would stay in float32);
    a ``source_column`` list of more than one name raises ``NotImplementedError`` (in the reference the second column lands in numpy's
    ``out=`` argument, an accident that is not reproduced); numpy's ``RuntimeWarning``s (log of zero, overflow) are not reproduced."""

    def __init__(self, **config: Any) -> None:
        if not config:
            raise ValueError("No columns to transform were specified.")
        spec = []
        for target, transform in config.items():
            if not isinstance(transform, dict) or "function" not in transform:
                raise ValueError(f"Invalid transformation specification for column {target}: {transform}")
            if transform["function"] not in obs.COLUMN_FUNCTIONS:  # before the sources, as the reference's constructor has it
                raise ValueError(f"Invalid transformation: {transform['function']}")
            source = transform.get("source_column", target)
            if not isinstance(source, str):
                source = tuple(source)
                if len(source) != 1:
                    raise NotImplementedError(f"column {target}: {len(source)} source columns {source}; every transformation takes one")
                source = source[0]
            spec.append((target, source, transform["function"]))
        self.transformations = spec
        column_ops_parity_note()

    def __repr__(self) -> str:
        return "ApplyColumnTransformations(" + ", ".join(f"{t}={f}({s})" for t, s, f in self.transformations) + ")"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        # obs.column_ops refuses a missing or non-numeric source on the host and only then looks for the device
        added = obs.column_ops(table, self.transformations)
        narrow = [s for s, dtype in obs.column_dtypes(table, self.transformations).items() if dtype_kind(dtype) == "f" and dtype.itemsize < 8]
        if narrow:
            say_once(LOG, (type(self), "float64"), "apply_column_transformations: float32 and float16 columns (here %s) are read as float64 and "
                     "the result is float64 (numpy would stay in float32)", narrow, level=logging.INFO)
        return t.with_columns(added)


# ---- row sets: sort_by, drop_duplicates, drop ------------------------------------------------------------------------------------------
class SortBy(Filter):
    """Sorts the rows of a table by the columns in ``columns`` (R: filters/tabular/sort_by.py:21-63: ``df.sort_values(by=columns,
    kind="stable")``): ascending by the key tuple, the first column most significant, missing values (NaN, NaT) of a key last, rows of
    equal tuples in table order.  The order is pandas', not IEEE's: ``-0.0`` and ``0.0`` tie, int64 keys compare as integers.  The
    permutation is computed on the device (``obs.sort_order``: ``atx_obs_order_key`` per column, one stable radix sort per key) and
    applied in one gather of all columns (``obs.take_rows`` -> ``atx_obs_take_rows``); a DataFrame is ``table.iloc[rows]``, so its index
    labels travel with the rows as in the reference.  A missing column raises ``ValueError``.

    Deviations: a key column that cannot be ordered (a uint64 column, objects without an order) raises ``ValueError`` — the reference
    logs the error and returns the frame unsorted; the caller's table is not modified."""

    def __init__(self, *, columns: list[str]) -> None:
        self.columns = [columns] if isinstance(columns, str) else list(columns)
        say_once(LOG, (type(self), "deviations"), "sort_by: a key column that cannot be ordered raises ValueError (the reference logs "
                 "the error and returns the table unsorted)", level=logging.INFO)

    def __repr__(self) -> str:
        return f"SortBy({self.columns})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        t.require(self.columns)
        if t.n_rows == 0 or not self.columns:
            return table.copy() if t.frame else dict(table)
        keys = [t[name] for name in self.columns]
        return t.take(obs.sort_order(keys, t.device, datetimes=[t.is_datetime(name) for name in self.columns]))


class DropDuplicates(Filter):
    """Keeps the first row, in table order, of every set of rows that are equal in a subset of the columns
    (R: filters/tabular/drop_duplicates.py:18-62: ``df.drop_duplicates(subset)``).  The subset is ``columns``, or every column whose name
    starts with ``column_prefix``, or — with neither — all columns; both at once raise ``ValueError`` at construction, a prefix that
    matches nothing and a missing column raise it at ``forward``.  Equality is pandas': ``-0.0`` equals ``0.0``, every NaN equals every
    NaN (NaT likewise), int64 compares as integers.  The rows are found on the device (``obs.first_rows``: keys, a stable sort,
    ``atx_obs_mark_first``) and taken in one gather of all columns (``obs.take_rows``); a DataFrame is ``table.iloc[rows]``.

    Deviations: a uint64 key column raises ``ValueError``; the caller's table is not modified."""

    def __init__(self, *, columns: list[str] | None = None, column_prefix: str | None = None) -> None:
        if bool(columns) and bool(column_prefix):
            raise ValueError("Either columns or column_prefix may be specified, but not both.")
        self.columns = [columns] if isinstance(columns, str) else columns
        self.column_prefix = column_prefix

    def __repr__(self) -> str:
        return f"DropDuplicates({self.columns if self.columns else (self.column_prefix + '*' if self.column_prefix else 'all columns')})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        if self.columns:
            subset = list(self.columns)
            t.require(subset)
        elif self.column_prefix:
            subset = [c for c in t.names if isinstance(c, str) and c.startswith(self.column_prefix)]
            if not subset:
                raise ValueError(f"No columns starting with '{self.column_prefix}' found in DataFrame.")
        else:
            subset = t.names
        if t.n_rows == 0 or not subset:
            return table.copy() if t.frame else dict(table)
        keys = [t[name] for name in subset]
        return t.take(obs.first_rows(keys, t.device, datetimes=[t.is_datetime(name) for name in subset]))


class Drop(Filter):
    """Removes the columns in ``columns`` from a table (R: filters/tabular/drop.py:18-48: ``df.drop(labels=columns, axis=1)``).  No
    columns raise ``ValueError`` at construction, a missing one at ``forward``.  Host bookkeeping: a DataFrame goes through pandas, a
    mapping gives a new dict without the names — the remaining columns are the caller's own objects, device tensors included; nothing
    is copied."""

    def __init__(self, *, columns: list[str]) -> None:
        if not columns:
            raise ValueError("No columns to drop were specified.")
        self.columns = [columns] if isinstance(columns, str) else list(columns)

    def __repr__(self) -> str:
        return f"Drop({self.columns})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        t.require(self.columns)
        return t.without(self.columns)


# ---- QC: masking, clipping, filling and dropping rows on the row-program kernel ----------------------------------------------------------
def _qc_note(kind: type) -> None:
    say_once(LOG, (kind, "table"), "%s: the caller's table is not modified (the reference writes into its argument); columns are read as "
             "float64 — exact for float32 and for integers below 2^53, beyond which nothing is specially handled", kind.__name__,
             level=logging.INFO)


def _dtypes(t: Table, names: Any) -> dict[str, Any]:
    return {name: (t[name].dtype if isinstance(t[name], torch.Tensor) else host_array(t[name]).dtype) for name in names}


def _torch_dtype(dtype: Any) -> torch.dtype:
    return dtype if isinstance(dtype, torch.dtype) else torch.from_numpy(np.empty(0, dtype=dtype)).dtype


def _narrowed(rows: dict[str, torch.Tensor], dtypes: dict[str, Any], integers: str) -> dict[str, torch.Tensor]:
    """The float64 result rows in the dtypes pandas hands back.  A float column keeps its dtype (the cast back is exact: every value is
    one of the column's own, a NaN, or a scalar rounded to the column's precision first).  An integer column, ``integers="nan"``: its
    own dtype and the caller's values — it is left out — when no row was masked, float64 otherwise; ``integers="whole"`` (clip): its own
    dtype when every clipped value is a whole number, float64 otherwise.  One reduction on the device decides either."""
    out = {}
    for name, row in rows.items():
        dtype = dtypes[name]
        if dtype_kind(dtype) == "f":
            out[name] = row if _torch_dtype(dtype) == torch.float64 else row.to(_torch_dtype(dtype))
        elif integers == "nan":
            if bool(torch.isnan(row).any()):
                out[name] = row
        elif bool((row == torch.floor(row)).all()):
            out[name] = row.to(_torch_dtype(dtype))
        else:
            out[name] = row
    return out


def _selected(t: Table, columns: list[str] | None, column_prefix: str | None) -> list[str] | None:
    """R: the ``columns`` / ``column_prefix`` selection every such filter repeats; None with neither."""
    if columns:
        t.require(columns)
        return list(columns)
    if column_prefix:
        found = [c for c in t.names if isinstance(c, str) and c.startswith(column_prefix)]
        if not found:
            raise ValueError(f"No columns starting with '{column_prefix}' found in DataFrame.")
        return found
    return None


class _MaskFilter(Filter):
    """What the masking filters share: compile, run, narrow, hand back through ``Table``."""

    integers = "nan"

    def _program(self, t: Table, dtypes: dict[str, Any]) -> obs.RowProgram:
        raise NotImplementedError

    def _columns(self, t: Table) -> list[str]:
        raise NotImplementedError

    def _rows(self, t: Table) -> dict[str, torch.Tensor]:
        return {}

    def forward(self, table: Any) -> Any:
        t = Table(table)
        dtypes = _dtypes(t, self._columns(t))
        program = self._program(t, dtypes)  # the host's errors come before anything touches the device
        if t.n_rows == 0 or not program.launches:
            return table.copy() if t.frame else dict(table)
        rows = obs.row_program(table, program, dev=t.device, rows=self._rows(t))
        return t.replaced(_narrowed(rows, dtypes, self.integers))


class MaskValues(_MaskFilter):
    """NaN where ``column OPERATOR value`` (R: filters/tabular/mask.py:36-87).  ``**config`` maps a column to ``{"value": v, "operator":
    op}``; ``op`` is one of ``> < == != >= <=`` or ``gt lt eq ne ge le`` and defaults to ``==``.  The constructor's ``ValueError``s are the
    reference's.  One launch per four columns (``obs.compile_mask_values`` -> ``obs.row_program`` -> ``atx_obs_column_ops``).  A float32 column
    is compared in float32, as numpy compares it (the value is rounded first), and stays float32; an integer column comes back
    unchanged when nothing was masked and float64 otherwise (pandas' rule).

    Deviations: the caller's table is not modified; integers beyond 2^53 are not specially handled; a bool column raises ``ValueError``."""

    def __init__(self, **config: Any) -> None:
        if not config:
            raise ValueError("No columns to mask were specified.")
        self.config = {}
        for col, condition in config.items():
            if not isinstance(condition, dict):
                raise ValueError(f"Mask condition for column {col} must be a dictionary, ")
            if "value" not in condition:
                raise ValueError(f"Mask condition for column {col} must contain a 'value' key.")
            operator = condition.get("operator", "==")
            if operator not in obs.MASK_OPERATORS:
                raise ValueError(f"Invalid operator '{operator}' for column {col}. "
                                 f"Valid operators are: {', '.join(obs.MASK_OPERATORS.keys())}.")
            self.config[col] = (operator, condition["value"])
        _qc_note(type(self))

    def __repr__(self) -> str:
        return "MaskValues(" + ", ".join(f"{c} {o} {v}" for c, (o, v) in self.config.items()) + ")"

    def _columns(self, t: Table) -> list[str]:
        t.require(list(self.config))
        return list(self.config)

    def _program(self, t: Table, dtypes: dict[str, Any]) -> obs.RowProgram:
        return obs.compile_mask_values(self.config, dtypes)


def _check_ranges(config: dict, what: str, noun: str) -> None:
    """R: mask_outside_range.py:40-50 and clip.py:44-52, word for word."""
    for column, bounds in config.items():
        if not isinstance(bounds, (list, tuple)) or len(bounds) != 2:
            raise ValueError(f"Invalid {what} range for column {column}: {bounds}")
        if not all(isinstance(v, (int, float)) or v is None for v in bounds):
            raise ValueError(f"{noun} range values for column {column} must be numeric or None: {bounds}")


class MaskOutsideRange(_MaskFilter):
    """NaN where ``column < low`` or ``column > high`` (R: filters/tabular/mask_outside_range.py:19-60).  ``**config`` maps a column to
    ``[low, high]``; None is no bound.  Numerics and dtypes as ``mask_tabular``.  A missing column raises ``ValueError`` (the reference: a
    ``KeyError`` from pandas)."""

    def __init__(self, **config: Any) -> None:
        if not config:
            raise ValueError("No columns to mask were specified.")
        _check_ranges(config, "mask", "Mask")
        self.config = config
        _qc_note(type(self))

    def __repr__(self) -> str:
        return f"MaskOutsideRange({self.config})"

    def _columns(self, t: Table) -> list[str]:
        t.require(list(self.config))
        return list(self.config)

    def _program(self, t: Table, dtypes: dict[str, Any]) -> obs.RowProgram:
        return obs.compile_mask_outside_range({c: tuple(r) for c, r in self.config.items()}, dtypes)


class MaskInfs(_MaskFilter):
    """NaN where a column is infinite (R: filters/tabular/mask_infs.py:21-64): ``|x| > DBL_MAX``.  ``columns`` or ``column_prefix``, exactly
    one of them (``ValueError`` otherwise, at construction)."""

    def __init__(self, *, columns: list[str] | None = None, column_prefix: str | None = None) -> None:
        if bool(columns) == bool(column_prefix):
            raise ValueError("Either columns or column_prefix must be specified, but not both.")
        self.columns = [columns] if isinstance(columns, str) else columns
        self.column_prefix = column_prefix
        _qc_note(type(self))

    def __repr__(self) -> str:
        return f"MaskInfs({self.columns if self.columns else self.column_prefix + '*'})"

    def _columns(self, t: Table) -> list[str]:
        return _selected(t, self.columns, self.column_prefix)

    def _program(self, t: Table, dtypes: dict[str, Any]) -> obs.RowProgram:
        return obs.compile_mask_beyond(list(dtypes), None, dtypes)


class MaskDewpointTemperature(_MaskFilter):
    """NaN in the dewpoint column — and, with ``mask_specific_humidity``, in the humidity column — where ``temperature < dewpoint``
    (R: filters/tabular/mask_dewpoint_temperature.py:20-73).  One condition, on the dewpoint as it came: a NaN dewpoint masks nothing."""

    def __init__(self, *, temperature: str = "2t", dewpoint_temperature: str = "2d", specific_humidity: str = "2q",
                 mask_specific_humidity: bool = False) -> None:
        self.temperature = temperature
        self.dewpoint_temperature = dewpoint_temperature
        self.specific_humidity = specific_humidity
        self.mask_specific_humidity = mask_specific_humidity
        _qc_note(type(self))

    def __repr__(self) -> str:
        return f"MaskDewpointTemperature({self.temperature!r} < {self.dewpoint_temperature!r})"

    def _columns(self, t: Table) -> list[str]:
        names = [self.temperature, self.dewpoint_temperature] + ([self.specific_humidity] if self.mask_specific_humidity else [])
        t.require(names)
        return names

    def _program(self, t: Table, dtypes: dict[str, Any]) -> obs.RowProgram:
        return obs.compile_mask_dewpoint(self.temperature, self.dewpoint_temperature,
                                         self.specific_humidity if self.mask_specific_humidity else None, dtypes)


def _epoch_day(value: Any) -> int:
    """``pd.to_datetime(str(value), format="%Y%m%d")`` as whole days since the epoch (R: exclude_dates.py:69-70)."""
    try:
        return (datetime.datetime.strptime(str(value), "%Y%m%d").date() - datetime.date(1970, 1, 1)).days
    except ValueError as e:
        raise ValueError(f"time data \"{value}\" doesn't match format \"%Y%m%d\": {e}") from None


class ExcludeDates(_MaskFilter):
    """NaN in a column where the row's ``date`` lies in one of the column's date ranges, both ends inclusive
    (R: filters/tabular/exclude_dates.py:21-91).  ``**config`` maps a column to a list of ``[start, end]`` (``YYYYMMDD`` as int or
    str); a single pair is one range.  The bounds are whole UTC days, so the condition is ``start_day <= day < end_day + 1`` with
    ``day = floor(date_ns / 86 400e9)``, computed once per call on the device (``obs.utc_days``; NaT is NaN and in no range); the ranges
    are compares in the program, OR-ed.  The constructor's ``ValueError``s are the reference's."""

    def __init__(self, **config: Any) -> None:
        if not config:
            raise ValueError("No columns to exclude dates from were specified.")
        self.excluded_dates: dict[str, list[tuple[int, int]]] = {}
        for column, ranges in config.items():
            if not (ranges and isinstance(ranges, (list, tuple))):
                raise ValueError(f"Invalid date ranges {ranges} for column '{column}'. Expected a list/tuple.")
            if len(ranges) == 2 and all(isinstance(r, (int, str)) for r in ranges):
                ranges = [ranges]  # a single pair
            for date_range in ranges:
                try:
                    start, end = date_range
                except (ValueError, TypeError) as e:
                    raise ValueError(f"Invalid date range {date_range} for column '{column}'. "
                                     "Expected a tuple like (start_date, end_date).") from e
                self.excluded_dates.setdefault(column, []).append((_epoch_day(start), _epoch_day(end)))
        _qc_note(type(self))

    def __repr__(self) -> str:
        return f"ExcludeDates({ {c: len(r) for c, r in self.excluded_dates.items()} })"

    def _columns(self, t: Table) -> list[str]:
        t.require(list(self.excluded_dates) + ["date"])
        return list(self.excluded_dates)

    def _program(self, t: Table, dtypes: dict[str, Any]) -> obs.RowProgram:
        if not (t.is_datetime("date") or column_kind(t["date"]) in "iO"):
            raise ValueError(f"the date column holds {column_kind(t['date'])!r} values, not datetimes")
        return obs.compile_exclude_dates(self.excluded_dates, dtypes)

    def _rows(self, t: Table) -> dict[str, torch.Tensor]:
        return {obs.DAY_ROW: obs.utc_days(t["date"], t.device)}


class RemoveExtremeValues(_MaskFilter):
    """Masks, or drops the rows with, values beyond ``±threshold`` (R: filters/tabular/remove_extreme_values.py:21-92).  The columns are
    ``columns`` or those starting with ``column_prefix`` (exactly one of the two), plus ``latitude`` and ``longitude``.  ``method="mask"``:
    NaN where ``|x| > threshold``.  ``method="drop"`` (the default): the rows where no column exceeds the threshold are kept (a NaN does
    not exceed it) — ``obs.keep_rows`` and one gather of every column (``Table.take``; ``iloc`` for a DataFrame, so index labels travel)."""

    def __init__(self, *, columns: list[str] | None = None, column_prefix: str | None = None, threshold: float = 1e10,
                 method: str = "drop") -> None:
        if method not in ("mask", "drop"):
            raise ValueError(f"Invalid method '{method}'. Must be either 'mask' or 'drop'.")
        if bool(columns) == bool(column_prefix):
            raise ValueError("Either columns or column_prefix must be specified, but not both.")
        self.method = method
        self.columns = [columns] if isinstance(columns, str) else columns
        self.column_prefix = column_prefix
        self.threshold = threshold
        _qc_note(type(self))

    def __repr__(self) -> str:
        return f"RemoveExtremeValues({self.method}, threshold={self.threshold})"

    def _columns(self, t: Table) -> list[str]:
        names = _selected(t, self.columns, self.column_prefix) + ["latitude", "longitude"]
        t.require(names)
        return list(dict.fromkeys(names))

    def _program(self, t: Table, dtypes: dict[str, Any]) -> obs.RowProgram:
        return obs.compile_mask_beyond(list(dtypes), self.threshold, dtypes)

    def forward(self, table: Any) -> Any:
        if self.method == "mask":
            return super().forward(table)
        t = Table(table)
        dtypes = _dtypes(t, self._columns(t))
        program = obs.compile_keep_not_beyond(list(dtypes), self.threshold, dtypes)
        if t.n_rows == 0:
            return table.copy() if t.frame else dict(table)
        return t.take(obs.keep_rows(table, program, dev=t.device))


class ClipTabular(_MaskFilter):
    """``column.clip(low, high)`` (R: filters/tabular/clip.py:20-60).  ``**config`` maps a column to ``[low, high]``; None is no bound.
    ``CLIP_LOW`` then ``CLIP_HIGH`` in one launch: a NaN stays, ``-0.0`` stays against a bound of 0.  pandas' own rules are kept: a NaN
    bound is no bound, bounds the wrong way round are swapped, a float32 column is clipped to the bound rounded to float32 and stays
    float32, and an integer column stays integer when every clipped value is a whole number — always so with integer bounds — and is
    float64 otherwise."""

    integers = "whole"

    def __init__(self, **config: Any) -> None:
        if not config:
            raise ValueError("No columns to clip were specified.")
        _check_ranges(config, "clip", "Clip")
        self.config = config
        _qc_note(type(self))

    def __repr__(self) -> str:
        return f"ClipTabular({self.config})"

    def _columns(self, t: Table) -> list[str]:
        t.require(list(self.config))
        return list(self.config)

    def _program(self, t: Table, dtypes: dict[str, Any]) -> obs.RowProgram:
        return obs.compile_clip({c: tuple(r) for c, r in self.config.items()}, dtypes)


class ImputeNaNsTabular(Filter):
    """``table.fillna(value)`` (R: filters/tabular/impute_nans.py:20-81).  ``value`` is a scalar or a dict per column.  ``columns`` /
    ``column_prefix`` (not both: ``ValueError``) are validated against the table and then — as in the reference, whose ``forward`` calls
    ``fillna`` on the WHOLE frame — select nothing: every column is filled.  Floating-point columns are filled on the device
    (``FILL_NAN``; a float32 column gets the value rounded to float32 and stays float32); integer columns have nothing to fill.  A
    datetime or non-numeric column goes through pandas' own ``fillna`` in a DataFrame; in a mapping it raises ``ValueError`` if it has
    a missing entry, and stays as it is otherwise."""

    def __init__(self, *, value: Any, columns: list[str] | None = None, column_prefix: str | None = None) -> None:
        if bool(columns) and bool(column_prefix):
            raise ValueError("Either columns or column_prefix may be specified, but not both.")
        self.value = value
        self.columns = [columns] if isinstance(columns, str) else columns
        self.column_prefix = column_prefix
        _qc_note(type(self))

    def __repr__(self) -> str:
        return f"ImputeNaNsTabular(value={self.value!r})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        if _selected(t, self.columns, self.column_prefix) is not None:
            say_once(LOG, (type(self), "subset"), "impute_nans_tabular: columns / column_prefix are checked against the table and then "
                     "ignored, as in the reference: its forward() calls fillna(value) on the whole frame", level=logging.INFO)
        per_column = isinstance(self.value, dict)
        asked = [name for name in t.names if not per_column or name in self.value]
        floats = [name for name in asked if not t.is_datetime(name) and column_kind(t[name]) == "f"]
        others = [name for name in asked if name not in floats and (t.is_datetime(name) or column_kind(t[name]) not in "iub")]
        if not t.frame:
            for name in others:
                if bool(t.missing(name, torch.device("cpu") if not isinstance(t[name], torch.Tensor) else t[name].device).any()):
                    raise ValueError(f"impute_nans_tabular: column {name!r} is not numeric and has missing entries; only a DataFrame's "
                                     "own fillna can fill it")
        dtypes = _dtypes(t, floats)
        program = obs.compile_fill_nans({name: (self.value[name] if per_column else self.value) for name in floats}, dtypes)
        filled = {}
        if t.n_rows and program.launches:
            filled = _narrowed(obs.row_program(table, program, dev=t.device), dtypes, "nan")
        out = t.replaced(filled) if (filled or not t.frame) else table.copy()
        if t.frame and others:
            out[others] = table[others].fillna({name: self.value[name] for name in others} if per_column else self.value)
        return out


class DropNaNsTabular(Filter):
    """``table.dropna(how=how, subset=...)`` (R: filters/tabular/drop_nans.py:21-73).  ``how``: ``"any"`` (default) or ``"all"``; the subset
    is ``columns``, or the columns starting with ``column_prefix`` (not both), or every column.  Floating-point columns are tested in the
    program (``IS_NAN``); any other column enters as the 0 / 1 row of ``Table.missing`` — NaT and None count, an integer column has
    none.  The kept rows are taken in one gather of every column (``obs.keep_rows`` -> ``Table.take``; ``iloc`` for a DataFrame)."""

    def __init__(self, *, how: str = "any", columns: list[str] | None = None, column_prefix: str | None = None) -> None:
        if how not in ("any", "all"):
            raise ValueError(f"DropNaNs - 'how' must be either 'any' or 'all', not '{how}'.")
        if bool(columns) and bool(column_prefix):
            raise ValueError("Either columns or column_prefix may be specified, but not both.")
        self.how = how
        self.columns = [columns] if isinstance(columns, str) else columns
        self.column_prefix = column_prefix
        _qc_note(type(self))

    def __repr__(self) -> str:
        return f"DropNaNsTabular(how={self.how!r})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        subset = _selected(t, self.columns, self.column_prefix)
        subset = t.names if subset is None else subset
        if t.n_rows == 0 or not subset:
            return table.copy() if t.frame else dict(table)
        kinds = {name: ("M" if t.is_datetime(name) else column_kind(t[name])) for name in subset}
        dtypes = {name: (np.dtype(np.float64) if kinds[name] == "f" else np.dtype(np.int64)) for name in subset}
        program = obs.compile_keep_not_missing(subset, self.how, dtypes)
        rows = {f"%missing:{name}": t.missing(name, t.device).to(torch.float64) for name in subset if kinds[name] != "f"}
        return t.take(obs.keep_rows(table, program, dev=t.device, rows=rows))


# ---- the query language: filter_query and mask_values_custom on the row-expression kernel ------------------------------------------------
def _query_dtypes(t: Table) -> dict[str, Any]:
    """Every column's dtype as the query compiler reads it: datetimes say so (an int64 tensor named ``date`` is one)."""
    return {name: (np.dtype("datetime64[ns]") if t.is_datetime(name) else dtype) for name, dtype in _dtypes(t, t.names).items()}


class FilterQuery(Filter):
    """``table.query(query)`` (R: filters/tabular/filter_query.py:19-92): the rows where the expression holds, in the table's order.  The
    language is pandas' (``query``: names, numbers, ``+ - * /``, ``abs``, compares and chains, ``in`` / ``not in`` lists, ``and or not``, ``&``
    / ``|``, backticks; a string column against string literals); the typing is numpy's, so a float32 column compares and computes in
    float32.  The expression is ONE launch that writes a bit per row (``obs.compile_query`` -> ``obs.query_rows`` -> ``native.obs_row_expr``,
    ``native.obs_keep_positions``); the kept rows are taken in one gather of every column (``Table.take``; ``iloc`` for a DataFrame).  Every
    error is the reference's ``ValueError("Invalid query expression: ...")``.

    Deviations: what pandas accepts beyond the language above (``@local``, ``//``, ``%``, ``**``, other functions, arithmetic on booleans,
    datetimes) raises that ``ValueError``; integers ride in float64 (exact below 2^53, never wrapped)."""

    def __init__(self, *, query: str) -> None:
        if not query:
            raise ValueError("Query expression cannot be empty")
        self.query = query
        _qc_note(type(self))

    def __repr__(self) -> str:
        return f"FilterQuery({self.query!r})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        try:
            program = obs.compile_query(self.query, _query_dtypes(t))
        except ValueError as e:
            raise ValueError(f"Invalid query expression: {self.query}. Error: {e}") from None
        return t.take(obs.query_rows(table, program, dev=t.device))


class MaskValuesCustom(_MaskFilter):
    """NaN in a column where a query-style condition over any columns holds (R: filters/tabular/mask_values_custom.py:20-67).  ``**config``
    maps a column to its condition, in the language of ``filter_query``.  Conditions apply IN ORDER: a later one sees an earlier one's
    masked column.  They are one launch when they fit one program (``query.compile_masks`` -> ``obs.eval_rows`` -> ``native.obs_row_expr``:
    sequential ``NAN_WHERE``s, the masked columns on the stack), one launch per condition otherwise.  Dtypes as ``mask_tabular``: a float
    column keeps its dtype, an integer column comes back float64 if a row was masked and unchanged otherwise.  A missing target column
    raises ``ValueError`` (``Table.require``), anything wrong with a condition the reference's ``ValueError("Invalid condition for column
    ...")``."""

    def __init__(self, **config: Any) -> None:
        if not config:
            raise ValueError("No columns to mask were specified.")
        self.config = dict(config)
        _qc_note(type(self))

    def __repr__(self) -> str:
        return f"MaskValuesCustom({self.config})"

    def _compile(self, conditions: list, dtypes: dict[str, Any]) -> obs.ExprProgram:
        try:
            return query.compile_masks(conditions, dtypes)
        except query.SplitNeeded:
            raise
        except ValueError as e:
            raise ValueError(f"Invalid condition for column '{conditions[-1][0]}': {conditions[-1][1]}. Error: {e}") from None

    def forward(self, table: Any) -> Any:
        t = Table(table)
        t.require(list(self.config))
        conditions = [(col, text) for col, text in self.config.items()]
        dtypes = _query_dtypes(t)
        for one in conditions:  # every condition's own errors first, by its own name, before anything touches the device
            self._compile([one], dtypes)
        try:
            programs = [self._compile(conditions, dtypes)]
        except ValueError:  # too large for one launch, or conditions that cannot share one: one launch each
            programs = None
        if t.n_rows == 0:
            return table.copy() if t.frame else dict(table)
        if programs is not None:
            return t.replaced(_narrowed(obs.eval_rows(table, programs[0], dev=t.device), dtypes, "nan"))
        current, done = dict(table) if not t.frame else {name: table[name] for name in t.names}, {}
        for col, text in conditions:
            rows = _narrowed(obs.eval_rows(current, self._compile([(col, text)], dtypes), dev=t.device), {col: dtypes[col]}, "nan")
            for name, row in rows.items():  # an integer column that lost a row is float64 from here on
                current[name], done[name], dtypes[name] = row, row, row.dtype
        return t.replaced(done)


# ---- station identifiers and column names -------------------------------------------------------------------------------------------
class EncodeStatids(Filter):
    """The station identifier column as int64 (R: filters/tabular/encode_statids.py:18-60): the base-36 value of the stripped,
    upper-cased identifier if it is made of ``0-9A-Z``, else the first four bytes of the MD5 digest of the stripped identifier.  The
    column is packed into a byte matrix and encoded in one launch (``obs.encode_statids`` -> ``atx_text_encode_statids``); rows the
    kernel leaves undecided (non-ASCII, an interior NUL, 13 or more base-36 characters) are the host's, ``last_host_rows`` of them in
    the last ``forward``.  After it the table has no string column left and stays on the device.  A missing column raises ``ValueError``.

    A value of 2^63 or more has no int64: a DataFrame then gets pandas' own answer for the whole column (``Series.apply``: uint64 or
    object), a mapping raises ``OverflowError``.

    Deviations: the caller's table is not modified; an entry that is not a ``str`` raises ``ValueError`` (the reference:
    ``AttributeError`` from ``.strip()``); a trailing U+0000 is lost in numpy's conversion of the column and so ignored."""

    def __init__(self, *, station_id: str = "statid") -> None:
        self.station_id = station_id
        self.last_host_rows = 0
        say_once(LOG, (type(self), "deviations"), "encode_statids: the caller's table is not modified (the reference writes into its "
                 "argument); an entry that is not a str raises ValueError (the reference: AttributeError); a trailing U+0000 of an "
                 "identifier is ignored", level=logging.INFO)

    def __repr__(self) -> str:
        return f"EncodeStatids({self.station_id})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        t.require([self.station_id])
        packed = text_matrix(t[self.station_id])  # a non-str entry raises here, before the device is looked up
        try:
            code, self.last_host_rows = obs.encode_statids(t[self.station_id], t.device, packed=packed)
        except OverflowError:
            if not t.frame:
                raise
            say_once(LOG, (type(self), "overflow"), "encode_statids: an identifier encodes to 2^63 or more; the whole column is pandas' "
                     "own answer (uint64 or object), computed on the host")
            self.last_host_rows = t.n_rows
            out = table.copy()
            out[self.station_id] = table[self.station_id].apply(obs.statid_to_int)
            return out
        return t.replaced({self.station_id: code})


class RenameTabular(Filter):
    """Renames columns of a table (R: filters/tabular/rename.py:18-45: ``df.rename(columns=columns)``).  ``columns`` maps old names to
    new ones; a missing old name raises ``ValueError``.  Host bookkeeping (``Table.replaced``): a DataFrame goes through pandas, a mapping
    gives a new dict in the same order whose columns are the caller's own objects, device tensors included; nothing is copied."""

    def __init__(self, *, columns: dict[str, str]) -> None:
        self.columns = dict(columns)

    def __repr__(self) -> str:
        return f"RenameTabular({self.columns})"

    def forward(self, table: Any) -> Any:
        t = Table(table)
        t.require(list(self.columns))
        return t.replaced({}, renamed=self.columns)


filter_registry.register("encode_statids", EncodeStatids)
filter_registry.register("rename_tabular", RenameTabular)
filter_registry.register("filter_query", FilterQuery)
filter_registry.register("mask_values_custom", MaskValuesCustom)
filter_registry.register("mask_tabular", MaskValues)
filter_registry.register("mask_outside_range", MaskOutsideRange)
filter_registry.register("mask_infs", MaskInfs)
filter_registry.register("mask_dewpoint_temperature", MaskDewpointTemperature)
filter_registry.register("exclude_dates", ExcludeDates)
filter_registry.register("remove_extreme_values", RemoveExtremeValues)
filter_registry.register("clip_tabular", ClipTabular)
filter_registry.register("impute_nans_tabular", ImputeNaNsTabular)
filter_registry.register("drop_nans_tabular", DropNaNsTabular)
filter_registry.register("sort_by", SortBy)
filter_registry.register("drop_duplicates", DropDuplicates)
filter_registry.register("drop", Drop)
filter_registry.register("apply_column_transformations", ApplyColumnTransformations)
filter_registry.register("fill_orography", FillHeights)
filter_registry.register("geopotential_to_height_tabular", GeopotentialToHeightTabular)
filter_registry.register("irregular_to_grid", IrregularToGrid)
filter_registry.register("assign_to_grid", AssignToGrid)
filter_registry.register("superob", SuperOb)
filter_registry.register("add_forcings", AddForcings)
filter_registry.register("add_azimuth", AddAzimuth)
filter_registry.register("add_msg_angles", AddMSGAngles)
filter_registry.register("radiance_to_brightness_temperature", RadianceToBrightnessTemperature)
filter_registry.register("add_healpix", AddHealpix)
