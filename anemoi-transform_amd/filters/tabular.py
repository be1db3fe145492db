"""irregular_to_grid / assign_to_grid: where a table of observations enters the field path (R: filters/tabular/).

``assign_to_grid`` adds the nearest grid point of every observation to the table; ``irregular_to_grid`` turns the table into one
gridded field per target time and column, NaN where nothing was observed.  The fields it returns are levels of ONE stack in
HBM (``obs.grid_observations``: ``atx_obs_best_per_cell`` + ``atx_obs_fill_stack``), so a following ``regrid`` or per-point
filter finds them resident.

A table is a pandas DataFrame (when pandas can be imported) or a plain mapping ``name -> 1-D array / device tensor``.

Deviations from the reference, each said once when it first matters (``core.say_once``):
  * rows are taken by POSITION.  The reference goes through index labels (``df.loc[idxmin]``): a table whose index has duplicate
    labels would duplicate rows there.
  * ``spatial_index`` must be an integer column, or a float column whose non-missing entries are whole numbers; missing entries
    are dropped, as ``groupby`` drops them.
  * value columns must be numeric: they are read as float64, as the reference's float64 grids read them.
  * ``"h<nside>"`` grids need healpy and raise ``NotImplementedError``.
The other tabular filters of the reference (pandas bookkeeping with no field output) are not built: DESIGN.md §7.
"""

from __future__ import annotations

import datetime
import logging
from collections.abc import Mapping
from typing import Any

import numpy as np
import torch

from .. import obs
from ..core import Filter, filter_registry, say_once
from ..fields import MISSING, Field, FieldList, new_field_from_stack
from ..grids import lookup

LOG = logging.getLogger(__name__)


def _is_dataframe(table: Any) -> bool:
    try:
        import pandas as pd
    except ImportError:
        return False
    return isinstance(table, pd.DataFrame)


def _column_names(table: Any) -> list[str]:
    if _is_dataframe(table):
        return list(table.columns)
    if isinstance(table, Mapping):
        return list(table.keys())
    raise TypeError(f"a table is a pandas DataFrame or a mapping name -> column, got {type(table).__name__}")


def _require(table: Any, names: list[str]) -> None:
    # R: filters/tabular/support/utils.py:18-21
    available = _column_names(table)
    missing = set(names) - set(available)
    if missing:
        raise ValueError(f"DataFrame is missing columns: {missing}. Available columns: {available}")


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
    if ns == obs.NAT:
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
        _require(table, ["date", "spatial_index", self.window_date_column] + list(self.columns))
        if _is_dataframe(table) and not table.index.is_unique:
            say_once(LOG, (type(self), "position"), "irregular_to_grid: the table's index has duplicate labels; rows are taken by "
                     "position here, the reference would repeat the rows of a duplicated label")
        cells = table["spatial_index"]
        kind = cells.dtype.is_floating_point if isinstance(cells, torch.Tensor) else getattr(np.asarray(cells).dtype, "kind", "") == "f"
        if kind:
            say_once(LOG, (type(self), "float-index"), "irregular_to_grid: spatial_index is a float column; whole numbers are "
                     "read as indices and missing entries dropped", level=logging.INFO)
        latitudes, longitudes = self._define_grid(self.grid)
        window_ns = obs.to_ns(table[self.window_date_column])
        targets = obs.unique_in_order(window_ns)
        stack = obs.grid_observations(table["date"], cells, [table[c] for c in self.columns], targets, n_cells=len(latitudes),
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
        _require(table, ["latitude", "longitude"])
        grid_lat, grid_lon = _named_grid(self.grid)
        lat, lon = table["latitude"], table["longitude"]
        if isinstance(lat, torch.Tensor):
            lat, lon = lat.cpu().numpy(), lon.cpu().numpy()
        distances, indices = obs.nearest_grid_index(grid_lat, grid_lon, lat, lon)
        added = {f"grid_index_{self.grid}": indices, "distance": distances}
        if _is_dataframe(table):
            return table.assign(**added)
        return {**table, **added}


filter_registry.register("irregular_to_grid", IrregularToGrid)
filter_registry.register("assign_to_grid", AssignToGrid)
