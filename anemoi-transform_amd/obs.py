"""Observation tables onto a grid, in HBM (R: filters/tabular/irregular_to_grid.py).

The reference loops over the target times on the host; per target it selects the rows of the window, scores them, keeps the
best row per ``spatial_index`` with a pandas ``groupby().idxmin()`` and writes its values into float64 grids of NaN.  Here the
table goes to the device once (a few columns of ``n_obs`` values), ``atx_obs_best_per_cell`` chooses the winning ROW of every
(target, cell) with two order-independent atomic minima, and ``atx_obs_fill_stack`` gathers the winners' values into ONE stack of
``n_time * n_cols`` levels — level ``t * n_cols + c`` is target ``t``, column ``c``, the reference's field order.

What this module restates on the host is the bookkeeping around those two launches: the window strings the reference hands to
``anemoi.utils.window.Window`` (``parse_window``), ``pd.Timedelta(time_freq)`` (``parse_frequency``), datetimes as int64
nanoseconds (``to_ns``), ``spatial_index`` as int64 cells (``to_cells``) and the targets in order of first appearance
(``unique_in_order``).  Arrays may be numpy arrays (uploaded) or device tensors (used in place).  The column readers
(``to_ns``, ``float_column``, ``host_array``, ``datetime_ns``), the device a launch runs on (``launch_device``) and ``take_rows`` live in
``tables`` and are imported here under the names this module has always offered them by.

The second half serves ``superob`` (R: filters/tabular/superob.py), which thins a raw table before it is gridded: ``key_codes`` and
``superob_groups`` turn key columns into rows in group order (torch on the device: one stable sort), ``group_means`` is pandas'
``groupby().mean()`` bit for bit (``atx_obs_group_mean``: one Kahan sum per group and column in row order) and ``group_nearest`` its
``groupby()["distance"].idxmin()`` (``atx_obs_group_argmin``).

The third part is the per-row derived columns that recipes put between those steps (R: filters/tabular/add_forcings.py, add_azimuth.py,
add_msg_angles.py, radiance_to_brightness_temperature.py): ``forcings``, ``view_angles`` and ``brightness_temperature``, one launch each
(``atx_obs_forcings``, ``atx_obs_view_angles``, ``atx_obs_planck_bt``) over columns that stay in HBM, and ``meteosat_position``, the
sub-satellite table of ``add_msg_angles`` (torch on the device).

The fourth is ``fill_orography`` (R: filters/tabular/fill_heights.py, support/utils.py:24-55): ``HeightGrid`` keeps an orography in HBM
with its axes sorted, and ``fill_heights`` replaces the missing station altitudes of a table by the nearest orography height in one
launch (``atx_obs_fill_heights``); rows with two equally near axis entries go back to the host's ``cKDTree``.

The fifth is ``apply_column_transformations`` (R: filters/tabular/apply_column_transformations.py): ``compile_column_program`` turns
the ordered list of (target, source, function) into runs of at most 16 operations, and ``column_ops`` launches each run once
(``atx_obs_column_ops``): a transformation that reads an earlier one's target takes it from a register, not from memory.

The sixth is the row sets of ``sort_by`` and ``drop_duplicates`` (R: filters/tabular/sort_by.py, drop_duplicates.py): ``order_keys``
turns a column into int64 keys that order and compare as pandas does (``atx_obs_order_key``), ``sort_order`` is the stable multi-key
permutation (the library's stable radix sort, one pass per key), ``first_rows`` the first row of every group of equal key tuples
(``atx_obs_mark_first``), and ``take_rows`` gathers every column of a table by one row list (``atx_obs_take_rows``).

The seventh is the tabular QC filters (R: filters/tabular/mask.py, mask_outside_range.py, mask_infs.py, mask_dewpoint_temperature.py,
exclude_dates.py, remove_extreme_values.py, clip.py, impute_nans.py, drop_nans.py): one small compiler per filter (``compile_mask_values``
.. ``compile_keep_not_missing``) turns its configuration and the column dtypes into a ``RowProgram`` — launches of at most 16 slots of the
row operations ``native.ROW_OPS``, pure host logic — ``row_program`` runs it (``atx_obs_column_ops``, the row-program kernel) and
``keep_rows`` lists the rows a row-dropping filter keeps.

The eighth is ``filter_query`` and ``mask_values_custom`` (R: filters/tabular/filter_query.py, mask_values_custom.py): ``compile_query``
turns pandas' query text into an ``ExprProgram`` (``query``: parser, numpy's typing, Sethi-Ullman postfix order), ``query_rows`` runs it and
lists the rows it keeps (``native.obs_row_expr``: one bit per row; ``native.obs_keep_positions``: their ascending positions), ``eval_rows`` returns its value rows.

The ninth is ``encode_statids`` (R: filters/tabular/encode_statids.py): the one string column of a table as int64, one launch over its
byte matrix (``native_text.encode_statids`` -> ``atx_text_encode_statids`` of the companion library), the rows the kernel leaves
undecided answered by ``statid_to_int`` on the host.
"""

from __future__ import annotations

import datetime
import logging
import re
from collections.abc import Mapping
from typing import Any, NamedTuple, Sequence

import numpy as np
import torch

from . import native
from . import query as _query
from . import stack as _stack
from .stack import COLUMNS, Stack
from .tables import NAT, datetime_ns, float_column, host_array, launch_device, take_rows, to_ns  # noqa: F401
from .tables import dtype_kind as _dtype_kind, gather as _take, on_device as _device  # the names this module, its tests and tools know them by

_LOG = logging.getLogger(__name__)
_UNIT_NS = {"s": 10**9, "m": 60 * 10**9, "h": 3600 * 10**9, "d": 86400 * 10**9}
_OFFSET = re.compile(r"^([+-]?)(\d+)([smhd])$")
_WINDOW = re.compile(r"^([(\[])([^,]*),([^,]*)([)\]])$")


class Window(NamedTuple):
    """``target + before_ns  <(=)  date  <(=)  target + after_ns``; an end is ``<=`` when its ``closed_*`` is true."""

    before_ns: int
    after_ns: int
    closed_before: bool
    closed_after: bool


def _offset_ns(text: str, whole: str) -> int:
    text = text.strip()
    if text in ("0", "+0", "-0"):
        return 0
    m = _OFFSET.match(text)
    if m is None:
        raise ValueError(f"window {whole!r}: cannot read the offset {text!r} (expected <+-n><s|m|h|d> or 0)")
    ns = int(m.group(2)) * _UNIT_NS[m.group(3)]
    return -ns if m.group(1) == "-" else ns


def parse_window(text: str) -> Window:
    """``"(-6h, 0]"``, ``"[-3h, +3h)"`` ...: the subset ``( | [  <+-n><unit>, <+-n><unit>  ) | ]`` with units s / m / h / d of the
    strings the reference passes to ``anemoi.utils.window.Window`` (R: irregular_to_grid.py:107-108).  A bare ``0`` is allowed;
    anything else raises ``ValueError`` naming the string."""
    if not isinstance(text, str):
        raise ValueError(f"window {text!r}: expected a string such as '(-6h, 0]'")
    m = _WINDOW.match(text.strip())
    if m is None:
        raise ValueError(f"window {text!r}: expected '(' or '[', two offsets separated by a comma, then ')' or ']'")
    before, after = _offset_ns(m.group(2), text), _offset_ns(m.group(3), text)
    if before > after:
        raise ValueError(f"window {text!r}: the first offset lies after the second")
    return Window(before, after, m.group(1) == "[", m.group(4) == "]")


def parse_frequency(freq: Any) -> int:
    """``pd.Timedelta(time_freq)`` in nanoseconds for ``"6h"``, ``"30m"``, ``"1d"``, ``"90s"`` (a ``timedelta`` /
    ``np.timedelta64`` is taken as it is).  Must be positive."""
    if isinstance(freq, datetime.timedelta):
        ns = (freq.days * 86400 + freq.seconds) * 10**9 + freq.microseconds * 1000
    elif isinstance(freq, np.timedelta64):
        ns = int(freq.astype("timedelta64[ns]").astype(np.int64))
    else:
        m = re.match(r"^\s*(\d+)\s*([smhd]|min)\s*$", str(freq), flags=re.I)
        if m is None:
            raise ValueError(f"time_freq {freq!r}: expected <n><s|m|h|d>")
        ns = int(m.group(1)) * _UNIT_NS[m.group(2).lower()[0]]
    if ns <= 0:
        raise ValueError(f"time_freq {freq!r} must be positive")
    return ns


def to_cells(column: Any) -> np.ndarray | torch.Tensor:
    """``spatial_index`` as int64.  An integer column is taken as it is; a float column must hold whole numbers, its missing
    (non-finite) entries become -1, which no grid has: ``groupby`` drops them in the reference."""
    if isinstance(column, torch.Tensor):
        c = column.reshape(-1)
        if c.dtype in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
            return c.to(torch.int64)
        if not c.dtype.is_floating_point:
            raise ValueError(f"spatial_index must be an integer or float column, got {c.dtype}")
        ok = torch.isfinite(c) & (c.abs() < 2.0**62)
        if bool((ok & (c != torch.floor(c))).any()):
            raise ValueError("spatial_index holds values that are not whole numbers")
        return torch.where(ok, c, torch.full_like(c, -1.0)).to(torch.int64)
    a = host_array(column).reshape(-1)
    if a.dtype.kind in "iu":
        return np.ascontiguousarray(a, dtype=np.int64)
    try:
        a = a.astype(np.float64)
    except (ValueError, TypeError):
        raise ValueError(f"spatial_index must be an integer or float column, got {a.dtype}") from None
    ok = np.isfinite(a) & (np.abs(a) < 2.0**62)
    if np.any(a[ok] != np.floor(a[ok])):
        raise ValueError("spatial_index holds values that are not whole numbers")
    return np.where(ok, a, -1.0).astype(np.int64)


def to_values(columns: Any) -> np.ndarray | torch.Tensor:
    """The value columns as ONE float64 ``[n_cols, n_obs]`` array (a device tensor if any column is one)."""
    if isinstance(columns, torch.Tensor):
        v = columns.reshape(1, -1) if columns.dim() == 1 else columns
        return v.to(torch.float64)
    if isinstance(columns, np.ndarray) and columns.ndim == 2:
        return np.ascontiguousarray(columns, dtype=np.float64)
    columns = list(columns)
    if any(isinstance(c, torch.Tensor) for c in columns):
        dev = next(c.device for c in columns if isinstance(c, torch.Tensor))
        rows = [c if isinstance(c, torch.Tensor) else torch.from_numpy(np.asarray(host_array(c), dtype=np.float64)) for c in columns]
        return torch.stack([r.reshape(-1).to(device=dev, dtype=torch.float64) for r in rows])
    try:
        rows = [np.asarray(host_array(c), dtype=np.float64).reshape(-1) for c in columns]
    except (ValueError, TypeError) as e:
        raise ValueError(f"value columns must be numeric (they are read as float64): {e}") from None
    if len({r.size for r in rows}) > 1:
        raise ValueError(f"value columns differ in length: {[r.size for r in rows]}")
    return np.stack(rows) if rows else np.zeros((0, 0))


def unique_in_order(ns: np.ndarray | torch.Tensor) -> np.ndarray:
    """The distinct values of an int64 column in order of FIRST APPEARANCE (``Series.unique()``), as a host array."""
    if isinstance(ns, torch.Tensor):
        if ns.numel() == 0:
            return np.zeros(0, dtype=np.int64)
        uniq, inverse = torch.unique(ns, sorted=True, return_inverse=True)
        first = torch.full((uniq.numel(),), ns.numel(), dtype=torch.int64, device=ns.device)
        first.scatter_reduce_(0, inverse, torch.arange(ns.numel(), device=ns.device), reduce="amin")
        return uniq[torch.argsort(first)].cpu().numpy()
    uniq, first = np.unique(ns, return_index=True)
    return uniq[np.argsort(first, kind="stable")]


def _prepare(date_ns, cell, values, target_ns, window, freq, weight, dev):
    dev = _stack.device() if dev is None else dev
    window = parse_window(window) if isinstance(window, str) else Window(*window)
    freq_ns = freq if isinstance(freq, (int, np.integer)) else parse_frequency(freq)
    if not 0.0 <= float(weight) <= 1.0:
        raise ValueError("nan_score_weight must be in the range [0.0, 1.0]")
    date_ns, cell, target_ns = _device(to_ns(date_ns), dev), _device(to_cells(cell), dev), _device(to_ns(target_ns), dev)
    values = to_values(values)
    values = _device(values, dev) if values.shape[1] > 0 else torch.empty(tuple(values.shape), dtype=torch.float64, device=dev)
    n_cols, n_obs = values.shape
    if n_cols == 0:
        raise ValueError("At least one column must be specified")
    if date_ns.numel() != n_obs or cell.numel() != n_obs:
        raise ValueError(f"columns differ in length: date {date_ns.numel()}, spatial_index {cell.numel()}, values {n_obs}")
    return date_ns, cell, values, target_ns, window, int(freq_ns), float(weight), dev


def _winners(date_ns, cell, values, target_ns, window, freq_ns, weight, n_cells, dev) -> torch.Tensor:
    n_time = target_ns.numel()
    best = torch.empty((n_time, n_cells), dtype=torch.int64, device=dev)
    winner = torch.empty((n_time, n_cells), dtype=torch.int32, device=dev)
    native.obs_best_per_cell(date_ns, cell, values, target_ns, best, winner, n_cells=n_cells, before_ns=window.before_ns,
                             after_ns=window.after_ns, closed_before=window.closed_before, closed_after=window.closed_after,
                             freq_ns=freq_ns, weight=weight)
    return winner


def best_per_cell(date_ns: Any, cell: Any, values: Any, target_ns: Any, *, n_cells: int, window: Any = "(-6h, 0]", freq: Any = "6h",
                  weight: float = 0.0, dev: torch.device | None = None) -> torch.Tensor:
    """``winner[t, c]`` (device int32 ``[n_time, n_cells]``): the row that target ``t`` shows in cell ``c``, -1 for none — the
    row of smallest score ``|date - target| / freq`` (``weight`` > 0: ``(1 - w) * that + w * nan_count / n_cols``) among the rows
    of the cell whose date lies in ``window`` around the target and whose values are not all NaN; among equal scores the first
    row of the table (R: irregular_to_grid.py:209-317)."""
    date_ns, cell, values, target_ns, window, freq_ns, weight, dev = _prepare(date_ns, cell, values, target_ns, window, freq, weight, dev)
    return _winners(date_ns, cell, values, target_ns, window, freq_ns, weight, int(n_cells), dev)


def grid_observations(date_ns: Any, cell: Any, values: Any, target_ns: Any, *, n_cells: int, window: Any = "(-6h, 0]",
                      freq: Any = "6h", weight: float = 0.0, layout: int = COLUMNS, dev: torch.device | None = None,
                      return_winner: bool = False) -> Stack | tuple[Stack, torch.Tensor]:
    """The float64 stack of ``n_time * n_cols`` levels over ``n_cells`` points whose level ``t * n_cols + c`` is column ``c`` of the
    best observation per cell for target ``t``, NaN where nothing was observed (R: irregular_to_grid.py:113-161).

    ``date_ns`` / ``target_ns``: datetimes or int64 nanoseconds; ``cell``: the grid index of every row; ``values``: the columns
    (a sequence of 1-D arrays or one ``[n_cols, n_obs]`` array).  numpy arrays are uploaded, device tensors used in place.
    ``window``: a string for ``parse_window`` or a ``Window``; ``freq``: a string for ``parse_frequency`` or nanoseconds."""
    date_ns, cell, values, target_ns, window, freq_ns, weight, dev = _prepare(date_ns, cell, values, target_ns, window, freq, weight, dev)
    n_cells, n_time, n_cols = int(n_cells), target_ns.numel(), values.shape[0]
    winner = _winners(date_ns, cell, values, target_ns, window, freq_ns, weight, n_cells, dev)
    out = Stack.empty(n_cells, n_time * n_cols, torch.float64, dev, layout)
    native.obs_fill_stack(winner, values, out.data, n_time=n_time, n_cells=n_cells, pitch=out.pitch, layout=layout)
    return (out, winner) if return_winner else out


def nearest_grid_index(grid_lat: np.ndarray, grid_lon: np.ndarray, lat: Any, lon: Any) -> tuple[np.ndarray, np.ndarray]:
    """``cKDTree(column_stack([grid_lat, grid_lon])).query(column_stack([lat, lon]))`` on the device: ``(distances, indices)`` of
    the nearest grid point in the PLANE of (latitude, longitude) degrees, not on the sphere (R: assign_to_grid.py:54-60).

    ``interp.device_knn`` searches points of [-1, 1]^3: both sets go in as ``(lat / 512, lon / 512, 0)``.  Scaling by a power of
    two is exact, so ``sqrt(d2) * 512`` is cKDTree's distance bit for bit, and rows with exactly equidistant grid points are handed
    to cKDTree itself (``ties="ckdtree"``)."""
    from .interp import device_knn

    def plane(a: Any, b: Any) -> np.ndarray:
        a, b = (np.asarray(host_array(x), dtype=np.float64).reshape(-1) for x in (a, b))
        return np.column_stack([a / 512.0, b / 512.0, np.zeros_like(a)])

    grid, points = plane(grid_lat, grid_lon), plane(lat, lon)
    if np.abs(grid).max(initial=0.0) > 1.0 or np.abs(points[np.isfinite(points)]).max(initial=0.0) > 1.0:
        raise ValueError("latitudes / longitudes beyond +-512 degrees")
    indices, d2, _ = device_knn(grid, points, 1)
    return np.sqrt(d2[:, 0]) * 512.0, indices[:, 0]


# ---- superob: rows -> groups -> pandas' group means (R: filters/tabular/superob.py:78-96) --------------------------------------
class Groups(NamedTuple):
    """The rows of a table in group order.  Group ``g`` (numbered by ascending key, NOT by appearance) holds the rows
    ``order[offsets[g]:offsets[g + 1]]``, ascending; ``first[g]`` is its first row and ``appearance`` lists the groups in the
    order in which their first rows appear in the table — pandas' ``groupby(sort=False)`` order."""

    order: torch.Tensor  # int32 [n_sel]
    offsets: torch.Tensor  # int64 [n_groups + 1]
    first: torch.Tensor  # int64 [n_groups]
    appearance: torch.Tensor  # int64 [n_groups]

    @property
    def n_groups(self) -> int:
        return self.first.numel()


_KEY_LIMIT = 2**62


def key_codes(column: Any) -> tuple[np.ndarray | torch.Tensor, np.ndarray | torch.Tensor | None]:
    """A key column as ``(int64 codes, valid)``: equal entries get equal codes, ``valid`` (None: every row) is false where the
    entry is missing (NaN, NaT, None) — ``groupby`` drops those rows.  Integer, bool and datetime columns and float columns of
    whole numbers are their own codes; anything else (strings, categoricals, other floats) is numbered on the host first."""
    if isinstance(column, torch.Tensor):
        c = column.reshape(-1)
        if not c.dtype.is_floating_point:
            return c.to(torch.int64), None
        ok = ~torch.isnan(c)
        whole = torch.isfinite(c) & (c.abs() < 2.0**62) & (c == torch.floor(c))
        if bool((whole | ~ok).all()):
            return torch.where(ok, c, torch.zeros_like(c)).to(torch.int64), ok
        codes = torch.zeros(c.numel(), dtype=torch.int64, device=c.device)
        codes[ok] = torch.unique(c[ok], return_inverse=True)[1]
        return codes, ok
    a = host_array(column).reshape(-1)
    if a.dtype.kind in "iub":
        return np.ascontiguousarray(a, dtype=np.int64), None
    if a.dtype.kind == "M":
        ns = to_ns(a)
        return ns, ns != NAT
    if a.dtype.kind == "f":
        a = a.astype(np.float64)
        ok = ~np.isnan(a)
        if np.all((np.isfinite(a) & (np.abs(a) < 2.0**62) & (a == np.floor(a))) | ~ok):
            return np.where(ok, a, 0.0).astype(np.int64), ok
        codes = np.zeros(a.size, dtype=np.int64)
        codes[ok] = np.unique(a[ok], return_inverse=True)[1]
        return codes, ok
    try:
        import pandas as pd

        codes = pd.factorize(column if hasattr(column, "dtype") and not isinstance(column, np.ndarray) else a)[0].astype(np.int64)
    except ImportError:
        seen: dict[Any, int] = {}
        codes = np.array([-1 if (v is None or v != v) else seen.setdefault(v, len(seen)) for v in a.tolist()], dtype=np.int64)
    return np.where(codes >= 0, codes, 0), codes >= 0


def superob_groups(keys: Sequence[Any], valid: Any = None, dev: torch.device | None = None) -> Groups:
    """The rows of a table grouped by the tuple of ``keys`` (int64 code columns, see ``key_codes``; numpy arrays are uploaded,
    device tensors used in place), rows where ``valid`` is false left out.  The bookkeeping is torch on the device: the key columns
    are folded into ONE int64 key, a STABLE sort of the kept rows by that key gives ``order``, the places where the sorted key
    changes give ``offsets``, and — the sort being stable — the first row of every segment is the group's first appearance."""
    dev = _stack.device() if dev is None else dev
    keys = [_device(k, dev).reshape(-1).to(torch.int64) for k in keys]
    if not keys:
        raise ValueError("at least one key column")
    n = keys[0].numel()
    if any(k.numel() != n for k in keys):
        raise ValueError(f"key columns differ in length: {[k.numel() for k in keys]}")
    if n >= 2**31:
        raise ValueError(f"{n} rows do not fit an int32 row index")
    rows = None
    if valid is not None:
        valid = _device(valid, dev).reshape(-1).to(torch.bool)
        if not bool(valid.all()):
            rows = torch.nonzero(valid).reshape(-1)
            keys = [k[rows] for k in keys]
    n_sel = keys[0].numel()
    if n_sel == 0:
        empty = torch.zeros(0, dtype=torch.int64, device=dev)
        return Groups(empty.to(torch.int32), torch.zeros(1, dtype=torch.int64, device=dev), empty, empty)
    key, span = None, 1
    for k in keys:
        lo, hi = int(k.min()), int(k.max())
        width = hi - lo + 1
        if key is None:
            key, span = k - lo, width
            continue
        if width >= _KEY_LIMIT or span * width >= _KEY_LIMIT:  # number both sides densely first (a sort each), then fold
            uk, key = torch.unique(key, return_inverse=True)
            uc, k = torch.unique(k, return_inverse=True)
            span, width, lo = uk.numel(), uc.numel(), 0
        key = key * width + (k - lo)
        span *= width
    sorted_key, perm = torch.sort(key, stable=True)
    change = torch.ones(n_sel, dtype=torch.bool, device=dev)
    change[1:] = sorted_key[1:] != sorted_key[:-1]
    starts = torch.nonzero(change).reshape(-1)
    offsets = torch.cat([starts, torch.tensor([n_sel], dtype=torch.int64, device=dev)])
    order = perm if rows is None else rows[perm]
    first = order[starts]
    return Groups(order.to(torch.int32).contiguous(), offsets.contiguous(), first, torch.argsort(first))


def group_means(values: torch.Tensor, groups: Groups) -> tuple[torch.Tensor, torch.Tensor]:
    """``(mean, count)``, float64 / int64 ``[n_cols, n_groups]`` in ``groups``' own numbering: pandas' ``groupby().mean()`` of the
    float64 device columns ``values`` (``[n_cols, n_obs]``) bit for bit — ``atx_obs_group_mean``."""
    n_cols = values.shape[0]
    mean = torch.empty((n_cols, groups.n_groups), dtype=torch.float64, device=values.device)
    count = torch.empty((n_cols, groups.n_groups), dtype=torch.int64, device=values.device)
    if n_cols and groups.n_groups:
        native.obs_group_mean(values, groups.order, groups.offsets, mean, count)
    return mean, count


def group_nearest(distance: torch.Tensor, groups: Groups) -> torch.Tensor:
    """Per group the first row of smallest ``distance`` (pandas ``groupby()["distance"].idxmin()`` on a table in row order), int64
    ``[n_groups]`` in ``groups``' own numbering — ``atx_obs_group_argmin``."""
    nearest = torch.empty(groups.n_groups, dtype=torch.int32, device=distance.device)
    if groups.n_groups:
        native.obs_group_argmin(distance.contiguous(), groups.order, groups.offsets, nearest)
    return nearest.to(torch.int64)


# ---- per-row derived columns (R: filters/tabular/add_forcings.py, add_azimuth.py, add_msg_angles.py, radiance_to_brightness_temperature.py) ----
FORCINGS = native.FORCINGS  # the nine names in the order of R: add_forcings.py:51-61, which is the order of the kernel's mask bits


def forcings(date: Any, latitude: Any, longitude: Any, columns: Sequence[str], dev: torch.device | None = None) -> dict[str, torch.Tensor]:
    """``{name: float64 device row}`` for the forcing names in ``columns`` (a subset of ``FORCINGS``), in the order given
    (R: add_forcings.py:68-127, support/compute_forcings.py:14-87) — ONE launch of ``atx_obs_forcings``; julian day, hours since
    midnight and the angles are computed once per row and shared by the outputs.  ``date``: datetimes or int64 nanoseconds (NaT gives
    NaN in every date-dependent column); ``latitude`` / ``longitude`` in degrees, read as float64."""
    unknown = set(columns) - set(FORCINGS)
    if unknown:
        raise ValueError(f"Unknown columns requested: {unknown}")
    dev = _stack.device() if dev is None else dev
    mask = 0
    for name in columns:
        mask |= 1 << FORCINGS.index(name)
    if mask == 0:
        return {}
    lat, lon = float_column(latitude, dev), float_column(longitude, dev)
    ns = _device(to_ns(date), dev)
    if not ns.numel() == lat.numel() == lon.numel():
        raise ValueError(f"columns differ in length: date {ns.numel()}, latitude {lat.numel()}, longitude {lon.numel()}")
    wanted = [name for name in FORCINGS if mask >> FORCINGS.index(name) & 1]
    out = torch.empty((len(wanted), ns.numel()), dtype=torch.float64, device=dev)
    native.obs_forcings(ns, lat, lon, mask, out)
    return {name: out[wanted.index(name)] for name in columns}


def view_angles(latitude: Any, longitude: Any, sat_latitude: Any, sat_longitude: Any, *, azimuth: bool = True, zenith: bool = True,
                dev: torch.device | None = None) -> dict[str, torch.Tensor]:
    """``{"azimuth": ..., "zenith": ...}`` (those asked for; float64 device rows, degrees) of a satellite at per-row
    ``(sat_latitude, sat_longitude)`` seen from ``(latitude, longitude)`` — ``atx_obs_view_angles``
    (R: support/sat_view_angles.py:52-97 calc_azimuth, :17-49 calc_zenith).  All four columns are read as float64."""
    dev = _stack.device() if dev is None else dev
    flags = (native.VIEW_AZIMUTH if azimuth else 0) | (native.VIEW_ZENITH if zenith else 0)
    if flags == 0:
        return {}
    cols = [float_column(c, dev) for c in (latitude, longitude, sat_latitude, sat_longitude)]
    if len({c.numel() for c in cols}) > 1:
        raise ValueError(f"columns differ in length: {[c.numel() for c in cols]}")
    names = [n for n, on in (("azimuth", azimuth), ("zenith", zenith)) if on]
    out = torch.empty((len(names), cols[0].numel()), dtype=torch.float64, device=dev)
    native.obs_view_angles(*cols, flags, out)
    return {name: out[k] for k, name in enumerate(names)}


# R: support/sat_view_angles.py:120-130 — (satellite id, day, the side of the day that counts, sub-satellite longitude)
_METEOSAT = ((55, "2016-10-20", ">", 41.5), (56, "2022-05-08", ">", 45.5), (57, "2013-01-24", "<", -3.4), (70, "2015-12-01", "<", -3.4))


def meteosat_position(satellite_id: Any, date: Any, dev: torch.device | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``(latitudes, longitudes)`` of the sub-satellite point per row (R: support/sat_view_angles.py:100-132), device tensors IN THE
    DTYPE OF THE ID COLUMN: the reference builds them with ``np.zeros_like(satids)``, so integer ids — which its own tests use —
    store 41.5 / 45.5 / -3.4 as 41 / 45 / -3, and the reference's literals depend on it.  The date comparisons are strict; NaT and
    unknown ids give 0."""
    dev = _stack.device() if dev is None else dev
    ids = satellite_id if isinstance(satellite_id, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(host_array(satellite_id)))
    ids = ids.reshape(-1).to(dev)
    ns = _device(to_ns(date), dev)
    if ids.numel() != ns.numel():
        raise ValueError(f"columns differ in length: satellite id {ids.numel()}, date {ns.numel()}")
    lons = torch.zeros_like(ids)
    for sat, day, side, lon in _METEOSAT:
        limit = int(np.datetime64(day, "ns").astype(np.int64))
        when = (ns > limit) if side == ">" else ((ns < limit) & (ns != NAT))
        value = torch.tensor(lon, dtype=torch.float64).to(ids.dtype)  # numpy's assignment into the id dtype: towards zero for integers
        lons = torch.where((ids == sat) & when, value.to(dev), lons)
    return torch.zeros_like(ids), lons


_C1_W, _C2 = 1.191042e-10, 1.4387768775  # W m^-2 sr^-1 cm^3; K cm (R: radiance_to_brightness_temperature.py:96-97)
_CRIS_BANDS = {"cris_fsr": ((1, 713, 650.0, 0.625), (714, 1578, 1210.0, 0.625), (1579, 2211, 2155.0, 0.625)),
               "cris_nsr": ((1, 713, 650.0, 0.625), (714, 1146, 1210.0, 1.250), (1147, 1305, 2155.0, 2.500))}


def cris_wavenumbers(channels: Any, mode: str) -> np.ndarray:
    """CrIS channel numbers to wavenumbers in cm^-1, NaN outside the bands of ``mode`` (R: radiance_to_brightness_temperature.py:52-80)."""
    if mode not in _CRIS_BANDS:
        raise ValueError(f"Invalid mode: {mode}. Must be 'cris_fsr' or 'cris_nsr'.")
    ch = np.asarray(channels, dtype=np.int64)
    nu = np.full(ch.shape, np.nan, dtype=float)
    for first, last, start, step in _CRIS_BANDS[mode]:
        m = (first <= ch) & (ch <= last)
        nu[m] = start + step * (ch[m] - first)
    return nu


def brightness_temperature(radiance: torch.Tensor, wavenumber: Any, out: torch.Tensor | None = None) -> torch.Tensor:
    """``b / log1p(a / max(R * 1e-2, 1e-300))`` with ``a = C1 nu^3``, ``b = C2 nu`` for a float64 device block ``radiance``
    ``[n_ch, n]`` in mW/(m^2 sr cm^-1), one row per channel of ``wavenumber`` (cm^-1; NaN gives NaN) — ``atx_obs_planck_bt``
    (R: radiance_to_brightness_temperature.py:96-113).  ``out`` may be ``radiance``."""
    nu = np.asarray(wavenumber, dtype=np.float64).reshape(-1)
    if radiance.dim() != 2 or radiance.shape[0] != nu.size:
        raise ValueError(f"radiance must be [n_ch, n] with one row per wavenumber, got {tuple(radiance.shape)} for {nu.size} channels")
    a, b = _device(_C1_W * (nu**3), radiance.device), _device(_C2 * nu, radiance.device)
    out = torch.empty_like(radiance) if out is None else out
    native.obs_planck_bt(radiance, a, b, out)
    return out


# ---- station heights from an orography (R: filters/tabular/fill_heights.py, support/utils.py:24-55 get_heights) ---------------------
FILL_SENTINEL = 9999.0  # R: fill_heights.py:80 — a station altitude of exactly 9999.0 is missing, as NaN is


def _check_axis(name: str, axis: Any) -> np.ndarray:
    a = np.asarray(host_array(axis))
    if a.ndim != 1 or a.size == 0:
        raise ValueError(f"orography {name} axis must be 1-D and non-empty, got shape {a.shape}")
    if a.dtype.kind not in "iuf":
        raise ValueError(f"orography {name} axis must be numeric, got dtype {a.dtype}")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError(f"orography {name} axis holds values that are not finite")
    return a


class HeightGrid:
    """An orography resident in HBM, as ``fill_heights`` searches it: both axes sorted ascending with the int32 permutations back to
    file order, and the heights in file order in their own dtype (float32 or float64; anything else numeric is widened to float64).
    Built once — the ``fill_orography`` filter keeps one per instance, as ``winds.py`` keeps its frame table.

    ``latitudes`` / ``longitudes``: 1-D, finite, non-empty, with distinct values, in any order; ``heights``: ``[n_lat, n_lon]``, a
    numpy array (uploaded) or a device tensor whose rows may be pitched (used in place).  Anything else raises ``ValueError`` before
    anything touches the device.  The host keeps the two axes for the rows whose nearest entry is a tie: those are answered by
    ``cKDTree`` itself, one tree per axis, built on first need (``tree``)."""

    def __init__(self, latitudes: Any, longitudes: Any, heights: Any, dev: torch.device | None = None) -> None:
        self.axes = (_check_axis("latitude", latitudes), _check_axis("longitude", longitudes))
        shape = tuple(heights.shape) if hasattr(heights, "shape") else np.shape(heights)
        if shape != (self.axes[0].size, self.axes[1].size):
            raise ValueError(f"orography heights have shape {shape}, the axes need {(self.axes[0].size, self.axes[1].size)}")
        self.order = tuple(np.argsort(a, kind="stable") for a in self.axes)
        self.sorted = tuple(a[o] for a, o in zip(self.axes, self.order))
        for name, s in zip(("latitude", "longitude"), self.sorted):
            if (np.diff(s) <= 0).any():  # -0.0 and 0.0 are one value
                raise ValueError(f"orography {name} axis repeats a value; which of the two the reference takes is arbitrary")
        if isinstance(heights, torch.Tensor):
            if heights.dtype not in (torch.float32, torch.float64) or (heights.stride(1) != 1 and shape[1] > 1):
                raise ValueError(f"device heights must be float32 or float64 with contiguous rows, got {heights.dtype}, strides {heights.stride()}")
            dev = heights.device if heights.is_cuda else (_stack.device() if dev is None else dev)
            self.heights = heights.to(dev)
        else:
            h = np.asarray(host_array(heights))
            if h.dtype.kind not in "iuf":
                raise ValueError(f"orography heights must be numeric, got dtype {h.dtype}")
            h = np.ascontiguousarray(h, dtype=h.dtype if h.dtype in (np.float32, np.float64) else np.float64)
            dev = _stack.device() if dev is None else dev
            self.heights = torch.from_numpy(h).to(dev)
        self.device = self.heights.device
        self.d_sorted = tuple(_device(s, self.device) for s in self.sorted)
        self.d_order = tuple(_device(o.astype(np.int32), self.device) for o in self.order)
        self._trees: list[Any] = [None, None]

    def tree(self, axis: int) -> Any:
        """The reference's ``cKDTree(np.c_[axis])`` over the axis in FILE order (0: latitude, 1: longitude), built once."""
        if self._trees[axis] is None:
            from scipy.spatial import cKDTree

            self._trees[axis] = cKDTree(np.c_[self.axes[axis]])
        return self._trees[axis]

    def nearest(self, axis: int, q: np.ndarray, tie: np.ndarray) -> np.ndarray:
        """File-order index of the entry nearest to every finite ``q``: cKDTree's own answer where ``tie``, elsewhere the strict
        arg-min of the float64 squares, which is cKDTree's whatever its build."""
        s, n = self.sorted[axis], self.sorted[axis].size
        hi = np.minimum(np.searchsorted(s, q, side="left"), n - 1)
        lo = np.maximum(hi - 1, 0)
        with np.errstate(over="ignore"):
            index = self.order[axis][np.where((s[lo] - q) * (s[lo] - q) < (s[hi] - q) * (s[hi] - q), lo, hi)]
        if tie.any():
            _, found = self.tree(axis).query(q[tie].reshape(-1, 1))
            if (found >= n).any():  # every square overflowed: cKDTree finds no neighbour, and the reference's indexing would raise
                raise ValueError(f"fill_heights: {int((found >= n).sum())} rows lie too far from the orography for a float64 distance")
            index[tie] = found
        return index


def fill_heights(grid: HeightGrid, latitude: Any, longitude: Any, altitude: Any, *, return_counts: bool = False) -> Any:
    """The station altitudes with the missing ones (NaN or 9999.0) taken from the orography ``grid``, a float64 device column — one
    launch of ``atx_obs_fill_heights`` (R: fill_heights.py:68-91, support/utils.py:24-55).  A row to fill gets ``heights[i, j]`` at
    the axis entries nearest to its latitude and longitude, each as ``cKDTree(np.c_[axis]).query`` decides it: no wrap-around in
    longitude, the end of the axis beyond it.  Every other row keeps its bits.  Rows the kernel flags — two equally near entries on
    an axis — are answered by ``grid.tree(axis)`` and one torch index into the resident heights, so every row is the reference's.

    Columns are numpy arrays, pandas Series or device tensors, read as float64.  A row to fill whose latitude or longitude is NaN
    or infinite raises ``ValueError`` naming how many there are (synchronises).  ``return_counts``: also ``(filled, flagged)``."""
    dev = grid.device
    lat, lon, alt = float_column(latitude, dev), float_column(longitude, dev), float_column(altitude, dev)
    n = alt.numel()
    if not lat.numel() == lon.numel() == n:
        raise ValueError(f"columns differ in length: latitude {lat.numel()}, longitude {lon.numel()}, altitude {n}")
    out = torch.empty(n, dtype=torch.float64, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    counters = torch.zeros(3, dtype=torch.int64, device=dev)
    native.obs_fill_heights(lat, lon, alt, grid.d_sorted[0], grid.d_order[0], grid.d_sorted[1], grid.d_order[1], grid.heights, out, flags,
                            counters)
    filled, flagged, bad = (int(c) for c in counters.cpu())
    if bad:
        raise ValueError(f"fill_heights: {bad} of {filled + bad} rows to fill have a latitude or longitude that is not finite")
    if flagged:
        rows = torch.nonzero(flags).reshape(-1)
        bits = flags[rows].cpu().numpy()
        i = grid.nearest(0, lat[rows].cpu().numpy(), (bits & native.FILL_TIE_LATITUDE) != 0)
        j = grid.nearest(1, lon[rows].cpu().numpy(), (bits & native.FILL_TIE_LONGITUDE) != 0)
        out[rows] = grid.heights[_device(i.astype(np.int64), dev), _device(j.astype(np.int64), dev)].to(torch.float64)
    return (out, (filled, flagged)) if return_counts else out


# ---- library functions over columns (R: filters/tabular/apply_column_transformations.py) --------------------------------------------
COLUMN_FUNCTIONS = tuple(native.COLUMN_OPS)  # the reference's ten names, in its order


class ColumnOp(NamedTuple):
    """One operation of a kernel step: ``target = function(source)``.  ``src``: the index, within the step, of the LATEST earlier
    operation whose target is ``source`` — its result is taken from a register — or -1: the column is read from memory.  ``store``:
    False where a later operation of the same step has the same target, so nothing is written."""
    function: str
    target: str
    source: str
    src: int
    store: bool


class KernelStep(NamedTuple):
    """One launch of ``atx_obs_column_ops``: 1 .. 16 operations."""
    ops: tuple[ColumnOp, ...]


class IntegerAbs(NamedTuple):
    """``abs`` of an integer column: it keeps its dtype, as ``np.abs`` does, so it runs outside the float64 kernel."""
    target: str
    source: str


def compile_column_program(spec: Sequence[tuple[str, str, str]], dtypes: Mapping[str, Any]) -> list[KernelStep | IntegerAbs]:
    """The ordered transformations ``[(target, source, function), ...]`` over a table whose columns have the (numpy or torch)
    ``dtypes``, as the steps that compute them: pure host logic.

    A ``KernelStep`` is a run of consecutive transformations, at most ``native.MAX_COLUMN_OPS``; within it a source that an earlier
    operation of the run wrote is that operation's result (``ColumnOp.src``), and a target that a later operation of the run writes
    again is not stored.  ``abs`` of a column that is integer AT THAT POINT (a table column, or the result of an earlier integer
    ``abs``) is an ``IntegerAbs`` and ends the run before it.  Between steps a column goes through memory.

    ``ValueError``: a function that is not one of ``COLUMN_FUNCTIONS``; a source that is bool, complex or not numeric.  ``KeyError``: a
    source that is neither a column of the table nor an earlier target."""
    kinds = {name: _dtype_kind(dt) for name, dt in dtypes.items()}
    steps: list[KernelStep | IntegerAbs] = []
    run: list[ColumnOp] = []

    def close() -> None:
        if run:
            last = {op.target: t for t, op in enumerate(run)}
            steps.append(KernelStep(tuple(op._replace(store=last[op.target] == t) for t, op in enumerate(run))))
            run.clear()

    for target, source, function in spec:
        if function not in native.COLUMN_OPS:
            raise ValueError(f"Invalid transformation: {function}")
        if source not in kinds:
            raise KeyError(f"DataFrame must contain columns {(source,)} for transformation.")
        if kinds[source] not in "iuf":
            raise ValueError(f"column {source!r}: a numeric column is needed, got dtype {dtypes.get(source, 'bool')}")
        if function == "abs" and kinds[source] in "iu":
            close()
            steps.append(IntegerAbs(target, source))
            kinds[target] = kinds[source]
            continue
        if len(run) == native.MAX_COLUMN_OPS:
            close()
        src = max((t for t, op in enumerate(run) if op.target == source), default=-1)
        run.append(ColumnOp(function, target, source, src, True))
        kinds[target] = "f"
    close()
    return steps


def column_dtypes(columns: Mapping[str, Any], spec: Sequence[tuple[str, str, str]]) -> dict[str, Any]:
    """The dtypes of the columns of the table that ``spec`` names as sources (``compile_column_program``'s second argument)."""
    names = {source for _, source, _ in spec} & set(columns.keys())
    return {name: (columns[name].dtype if isinstance(columns[name], torch.Tensor) else host_array(columns[name]).dtype) for name in names}


def column_ops(columns: Mapping[str, Any], spec: Sequence[tuple[str, str, str]], dev: torch.device | None = None) -> dict[str, torch.Tensor]:
    """``{target: device row}`` of the transformations ``[(target, source, function), ...]`` applied in order to the table ``columns``
    (a mapping or DataFrame of numpy arrays, pandas Series or device tensors), in the order the targets first appear
    (R: apply_column_transformations.py:55-61, :132-138).  One launch of ``atx_obs_column_ops`` per ``KernelStep`` of
    ``compile_column_program``; a repeated target is fine, the last one stands.

    Sources are read as float64 (``float_column``: a float64 device tensor is used in place, integers convert as numpy's cast does)
    and results are float64 — except ``abs`` of an integer column, which keeps its dtype (``torch.abs``).  The caller's columns are
    never written: every target, one equal to its source included, is a fresh row."""
    spec = [tuple(item) for item in spec]
    steps = compile_column_program(spec, column_dtypes(columns, spec))  # the host's errors come before anything touches the device
    dev = launch_device((columns[name] for name in columns.keys()), dev)
    current: dict[str, Any] = {}  # the targets written so far
    as_float: dict[str, torch.Tensor] = {}  # float64 device rows of the columns read so far

    def row(name: str) -> torch.Tensor:
        if name not in as_float:
            as_float[name] = float_column(current[name] if name in current else columns[name], dev)
        return as_float[name]

    for step in steps:
        if isinstance(step, IntegerAbs):
            col = current[step.source] if step.source in current else columns[step.source]
            if not isinstance(col, torch.Tensor):
                col = torch.from_numpy(np.ascontiguousarray(host_array(col)).reshape(-1))
            col = col.reshape(-1).to(dev)
            # an unsigned column is its own absolute value (torch has no abs for most unsigned types)
            written = {step.target: col.clone() if _dtype_kind(col.dtype) == "u" else torch.abs(col)}
        else:
            inputs = [row(op.source) if op.src < 0 else None for op in step.ops]
            lengths = {c.numel() for c in inputs if c is not None}
            if len(lengths) > 1:
                raise ValueError(f"columns differ in length: { {op.source: c.numel() for op, c in zip(step.ops, inputs) if c is not None} }")
            n = lengths.pop()  # the first operation of a step always reads memory
            outs = [torch.empty(n, dtype=torch.float64, device=dev) if op.store else None for op in step.ops]
            native.obs_column_ops([(native.COLUMN_OPS[op.function], op.src, c, o) for op, c, o in zip(step.ops, inputs, outs)], n)
            written = {op.target: o for op, o in zip(step.ops, outs) if op.store}
        for name, col in written.items():
            current[name] = col
            as_float.pop(name, None)
    return {target: current[target] for target in dict.fromkeys(t for t, _, _ in spec)}


# ---- row sets: pandas' order and equality on the device (R: filters/tabular/sort_by.py, drop_duplicates.py) --------------------------
def _host_ranks(column: Any) -> np.ndarray:
    """A non-numeric host column (strings, categoricals, objects) as int64 ranks: equal entries get equal ranks, the ranks ascend as
    pandas orders the entries, and every missing entry (None, NaN, NaT) gets ONE rank above all others — missing last, and equal to
    each other, as ``sort_values`` and ``drop_duplicates`` have it.  A categorical ranks by its categories' order, as pandas sorts it.
    Entries that cannot be ordered (a column mixing strings and numbers) raise ``ValueError``."""
    if hasattr(column, "cat"):
        codes = np.asarray(column.cat.codes, dtype=np.int64)
        return np.where(codes < 0, len(column.cat.categories), codes)
    a = host_array(column).reshape(-1)
    try:
        try:
            import pandas as pd

            codes, uniques = pd.factorize(a, sort=True)
            codes, n_unique = np.asarray(codes, dtype=np.int64), len(uniques)
            sorted(np.asarray(uniques, dtype=object).tolist())  # factorize puts numbers before strings; sort_values refuses the mix
        except ImportError:
            ok = np.array([not (v is None or v != v) for v in a.tolist()], dtype=bool)
            codes = np.full(a.size, -1, dtype=np.int64)
            uniques, codes[ok] = np.unique(a[ok], return_inverse=True)
            n_unique = len(uniques)
    except TypeError as e:
        raise ValueError(f"a key column of dtype {a.dtype} holds entries that cannot be ordered: {e}") from None
    return np.where(codes < 0, n_unique, codes)


def order_keys(column: Any, dev: torch.device | None = None, *, datetime: bool = False) -> torch.Tensor:
    """The int64 device keys of one column by pandas' order and equality (``atx_obs_order_key``): ``key(a) < key(b)`` exactly when
    ``sort_values`` puts a before b, ``key(a) == key(b)`` exactly when ``drop_duplicates`` takes them for the same value.  ``-0.0`` and
    ``0.0`` are one key; every NaN and NaT is one key, the largest; int64 compares as integers.  (One date shares NaT's key: INT64_MAX
    nanoseconds, pandas' ``Timestamp.max``.)

    float64, float32, int64, int32, int16, int8, uint8 and bool columns go to the kernel as they are; float16, uint16 and uint32 are
    widened exactly first; datetime64 / timedelta64 arrays are int64 nanoseconds with NaT (``datetime=True`` says the same of an int64
    tensor); uint64 raises ``ValueError`` (it has no int64 key).  Non-numeric columns exist only on the host and are ranked there
    (``pd.factorize(sort=True)``, missing last); their ranks take the int64 route.  numpy arrays are uploaded, device tensors used in place."""
    code = None
    if isinstance(column, torch.Tensor):
        c = column.reshape(-1)
        if datetime:
            if c.dtype != torch.int64:
                raise ValueError(f"a date tensor must hold int64 nanoseconds, got {c.dtype}")
            code = native.KEY_DATETIME
        elif c.dtype in (torch.float16, torch.bfloat16):
            c = c.to(torch.float32)
        elif c.dtype in (torch.uint16, torch.uint32):
            c = c.to(torch.int64)
        elif c.dtype not in native.KEY_DTYPES:
            raise ValueError(f"a {c.dtype} column has no int64 order key")
        dev = launch_device([c], None if c.is_cuda else dev)  # a device tensor is used where it is
        c = c.to(dev).contiguous()
    else:
        dev = launch_device((), dev)
        a = None if hasattr(column, "cat") else host_array(column).reshape(-1)
        if a is None or a.dtype.kind not in "iufbMm":
            a = _host_ranks(column)
        elif a.dtype.kind in "Mm":
            a = datetime_ns(a)
            code = native.KEY_DATETIME
        elif a.dtype.kind == "u" and a.dtype.itemsize == 8:
            raise ValueError("a uint64 column has no int64 order key")
        elif a.dtype.kind == "u" and a.dtype.itemsize > 1:
            a = a.astype(np.int64)
        elif a.dtype.kind == "f" and a.dtype.itemsize == 2:
            a = a.astype(np.float32)
        elif a.dtype.kind == "f" and a.dtype.itemsize > 8:
            raise ValueError(f"a {a.dtype} column has no int64 order key")
        if datetime and code is None:
            if a.dtype != np.int64:
                raise ValueError(f"a date column must hold datetimes or int64 nanoseconds, got {a.dtype}")
            code = native.KEY_DATETIME
        c = _device(a.astype(a.dtype.newbyteorder("="), copy=False), dev)
    key = torch.empty(c.numel(), dtype=torch.int64, device=dev)
    native.obs_order_key(c, key, code)
    return key


def _row_keys(columns: Sequence[Any], dev: torch.device | None, datetimes: Sequence[bool] | None) -> list[torch.Tensor]:
    columns = list(columns)
    if not columns:
        raise ValueError("at least one key column")
    dev = launch_device(columns, dev)
    flags = [False] * len(columns) if datetimes is None else list(datetimes)
    keys = [order_keys(c, dev, datetime=bool(f)) for c, f in zip(columns, flags)]
    if len({k.numel() for k in keys}) > 1:
        raise ValueError(f"key columns differ in length: {[k.numel() for k in keys]}")
    return keys


def _sort_keys(keys: Sequence[torch.Tensor]) -> torch.Tensor:
    """The stable ascending order of the rows by the tuple of int64 ``keys``, first key most significant: ONE STABLE SORT PER KEY, from
    the last key to the first (a radix sort by digits; the library's ``torch.sort(stable=True)`` on int64).  Between two sorts the next
    key is brought into the current order and the order composed with ``atx_obs_take_rows``."""
    order = None
    for key in reversed(list(keys)):
        if order is None:
            order = torch.sort(key, stable=True).indices
        else:  # rows already ordered by the later keys: a stable sort by this one keeps that order among its equals
            (moved,) = _take([key], order, check=False)
            (order,) = _take([order], torch.sort(moved, stable=True).indices, check=False)
    return order.contiguous()


def sort_order(columns: Sequence[Any], dev: torch.device | None = None, *, datetimes: Sequence[bool] | None = None) -> torch.Tensor:
    """The int64 device permutation that ``df.sort_values(by=columns, kind="stable")`` applies (R: filters/tabular/sort_by.py:51):
    rows ascending by the key tuple, the first column most significant, missing values (NaN, NaT) of a key last, rows of equal tuples
    in table order.  ``columns``: the key columns themselves (see ``order_keys``); ``datetimes[k]`` marks an int64 column as
    nanoseconds with NaT.  One stable sort per key, from the last to the first (``_sort_keys``) — a folded single key, as
    ``superob_groups`` builds it, would give the same permutation but needs the ranges of every key first."""
    return _sort_keys(_row_keys(columns, dev, datetimes))


def first_rows(columns: Sequence[Any], dev: torch.device | None = None, *, datetimes: Sequence[bool] | None = None) -> torch.Tensor:
    """The ascending int64 device row numbers that ``df.drop_duplicates(subset)`` keeps (R: filters/tabular/drop_duplicates.py:61): the
    first row, in table order, of every set of rows equal in ``columns`` by pandas' equality (``order_keys``).  The rows are sorted
    stably by the key tuple (``_sort_keys``), ``atx_obs_mark_first`` marks every row whose tuple differs from its predecessor's in
    that order — 16 keys per launch, further launches accumulating — and the marked rows are listed ascending."""
    keys = _row_keys(columns, dev, datetimes)
    n = keys[0].numel()
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=keys[0].device)
    order = _sort_keys(keys)
    keep = torch.empty(n, dtype=torch.uint8, device=order.device)
    for j in range(0, len(keys), native.MAX_ROWSET_COLUMNS):
        native.obs_mark_first(keys[j:j + native.MAX_ROWSET_COLUMNS], order, keep, accumulate=j > 0)
    return torch.nonzero(keep).reshape(-1)


# ---- row programs: the tabular QC filters (R: filters/tabular/mask.py, mask_outside_range.py, mask_infs.py, --------------------------
# ---- mask_dewpoint_temperature.py, exclude_dates.py, remove_extreme_values.py, clip.py, impute_nans.py, drop_nans.py) ---------------
DBL_MAX = float(np.finfo(np.float64).max)
DAY_NS = 86400 * 10**9
DAY_ROW = "%day"    # the whole UTC day of every row's date, float64 with NaT as NaN (``utc_days``)
KEEP_ROW = "%keep"  # the 0 / 1 row a keep-row program ends in
# R: mask.py:20-33, the 12 spellings
MASK_OPERATORS = {">": "cmp_gt", "<": "cmp_lt", "==": "cmp_eq", "!=": "cmp_ne", ">=": "cmp_ge", "<=": "cmp_le",
                  "gt": "cmp_gt", "lt": "cmp_lt", "eq": "cmp_eq", "ne": "cmp_ne", "ge": "cmp_ge", "le": "cmp_le"}
ROW_BINARY = frozenset(name for name, code in native.ROW_OPS.items() if code >= native.ROW_OPS["cmp_gt"])


class RowSlot(NamedTuple):
    """One operation of a launch of the row-program kernel.  ``op``: a ``native.ROW_OPS`` name.  x is the result of slot ``src`` of the
    same launch, or with ``src`` -1 the row ``read`` from memory, or for ``"scalar"`` the entry ``scalar`` of the program's scalars.  y, for
    a binary operation, is the result of the slot before.  ``store``: the row the result is written to, or None."""
    op: str
    src: int
    read: str | None
    scalar: int | None
    store: str | None


class RowLaunch(NamedTuple):
    """One launch of ``atx_obs_column_ops`` with codes of the second family: 1 .. 16 slots."""
    slots: tuple[RowSlot, ...]


class RowProgram(NamedTuple):
    """What a QC filter computes for one table: ``scalars`` (uploaded once per call), the ``launches`` in order, and the names of the rows
    that leave it (``results``).  A name starting with ``%`` is no column of the table: ``%day``, ``%missing:<column>`` are rows the
    caller provides, every other one an intermediate that crosses a launch boundary through a float64 device row."""
    scalars: tuple[float, ...]
    launches: tuple[RowLaunch, ...]
    results: tuple[str, ...]


class _RowBuilder:
    """Packs UNITS of slots into launches.  A unit is a list of ``(op, x, store)`` that stays together, because its binary operations
    take the slot before them: ``x`` is a row name (read from memory, or taken from the slot of this launch that last stored or copied
    that row), an int (a slot of the unit, counted from its start) or a 1-tuple (the number of a scalar)."""

    def __init__(self) -> None:
        self.scalars: list[float] = []
        self.launches: list[list[RowSlot]] = []
        self.run: list[RowSlot] = []
        self.where: dict[str, int] = {}  # row name -> the slot of the open launch that holds its current value

    def scalar(self, value: float) -> tuple[int]:
        self.scalars.append(float(value))
        return (len(self.scalars) - 1,)

    def close(self) -> None:
        if self.run:
            self.launches.append(self.run)
            self.run, self.where = [], {}

    def emit(self, unit: Sequence[tuple[str, Any, str | None]]) -> None:
        assert 0 < len(unit) <= native.MAX_COLUMN_OPS and unit[0][0] not in ROW_BINARY
        if len(self.run) + len(unit) > native.MAX_COLUMN_OPS:
            self.close()
        base = len(self.run)
        for op, x, store in unit:
            t = len(self.run)
            if isinstance(x, tuple):
                slot = RowSlot(op, -1, None, x[0], store)
            elif isinstance(x, int):
                slot = RowSlot(op, base + x, None, None, store)
            else:
                held = self.where.get(x, -1)
                slot = RowSlot(op, held, x if held < 0 else None, None, store)
                if op == "copy" and held < 0:
                    self.where[x] = t  # loaded once: later reads of this launch take the register
            self.run.append(slot)
            if store is not None:
                self.where[store] = t

    def finish(self, results: Sequence[str]) -> RowProgram:
        self.close()
        launches = []
        for k, run in enumerate(self.launches):
            last = {slot.store: t for t, slot in enumerate(run) if slot.store is not None}
            later = {slot.read for other in self.launches[k + 1:] for slot in other if slot.read is not None}
            # a row is written by the last slot of the launch that stores it, and an intermediate only where a later launch reads it
            launches.append(RowLaunch(tuple(
                slot._replace(store=slot.store if slot.store is not None and last[slot.store] == t
                              and (not slot.store.startswith("%") or slot.store in later or slot.store in results) else None)
                for t, slot in enumerate(run))))
        return RowProgram(tuple(self.scalars), tuple(launches), tuple(results))


def round_scalar(value: Any, dtype: Any) -> float:
    """The configured number as the column's compare sees it: numpy compares a float32 (float16) column with a Python number in the
    column's precision, so the number is rounded to it first — after that the float64 compare IS the narrow one.  float64 and integer
    columns take ``float(value)`` (an integer beyond 2^53 is rounded: not specially handled)."""
    if _dtype_kind(dtype) == "f":
        if isinstance(dtype, torch.dtype):
            return float(torch.tensor(float(value), dtype=torch.float64).to(dtype)) if dtype != torch.float64 else float(value)
        if np.dtype(dtype).itemsize < 8:
            with np.errstate(over="ignore"):
                return float(np.dtype(dtype).type(value))
    return float(value)


def _numeric(dtypes: Mapping[str, Any], name: str) -> Any:
    if _dtype_kind(dtypes[name]) not in "iuf":
        raise ValueError(f"column {name!r}: a numeric column is needed, got dtype {dtypes[name]}")
    return dtypes[name]


def compile_mask_values(conditions: Mapping[str, tuple[str, Any]], dtypes: Mapping[str, Any]) -> RowProgram:
    """``column -> (operator, value)``: NaN where ``column OPERATOR value`` (R: mask.py: ``col.mask(op(col, value))``)."""
    b = _RowBuilder()
    for col, (operator, value) in conditions.items():
        k = b.scalar(round_scalar(value, _numeric(dtypes, col)))
        b.emit([("copy", col, None), ("scalar", k, None), (MASK_OPERATORS[operator], 0, None), ("nan_where", 0, col)])
    return b.finish(list(conditions))


def compile_mask_outside_range(ranges: Mapping[str, tuple[Any, Any]], dtypes: Mapping[str, Any]) -> RowProgram:
    """``column -> (low, high)``: NaN where ``column < low`` or ``column > high``; None is no bound (R: mask_outside_range.py)."""
    b = _RowBuilder()
    results = []
    for col, (low, high) in ranges.items():
        dtype = _numeric(dtypes, col)
        if low is None and high is None:
            continue  # Series.mask(False): the column as it is
        unit: list[tuple[str, Any, str | None]] = [("copy", col, None)]
        if low is not None:
            unit += [("scalar", b.scalar(round_scalar(low, dtype)), None), ("cmp_lt", 0, None)]
        if high is not None:
            unit += [("scalar", b.scalar(round_scalar(high, dtype)), None), ("cmp_gt", 0, None)]
        if low is not None and high is not None:
            unit.append(("or", 2, None))
        b.emit(unit + [("nan_where", 0, col)])
        results.append(col)
    return b.finish(results)


def compile_mask_beyond(columns: Sequence[str], threshold: float | None, dtypes: Mapping[str, Any]) -> RowProgram:
    """NaN where ``|column| > threshold`` (R: remove_extreme_values.py, method ``mask``: the threshold is compared in the column's
    precision); ``threshold=None`` is ``mask_infs``: ``|column| > DBL_MAX``, not rounded — a float32 infinity is a float64 infinity."""
    b = _RowBuilder()
    for col in dict.fromkeys(columns):
        k = b.scalar(DBL_MAX if threshold is None else round_scalar(threshold, _numeric(dtypes, col)))
        _numeric(dtypes, col)
        b.emit([("copy", col, None), ("scalar", k, None), ("abs_gt", 0, None), ("nan_where", 0, col)])
    return b.finish(list(dict.fromkeys(columns)))


def compile_mask_dewpoint(temperature: str, dewpoint: str, humidity: str | None, dtypes: Mapping[str, Any]) -> RowProgram:
    """ONE condition, ``temperature < dewpoint`` on the original dewpoint, masks the dewpoint and — if named — the humidity
    (R: mask_dewpoint_temperature.py): a NaN dewpoint masks nothing."""
    for name in (temperature, dewpoint) + ((humidity,) if humidity else ()):
        _numeric(dtypes, name)
    b = _RowBuilder()
    unit: list[tuple[str, Any, str | None]] = [("copy", dewpoint, None), ("cmp_lt", temperature, None), ("nan_where", 0, dewpoint)]
    if humidity:
        unit += [("copy", 1, None), ("nan_where", humidity, humidity)]
    b.emit(unit)
    return b.finish([dewpoint] + ([humidity] if humidity else []))


def compile_exclude_dates(excluded: Mapping[str, Sequence[tuple[int, int]]], dtypes: Mapping[str, Any]) -> RowProgram:
    """``column -> [(start_day, end_day), ...]`` in whole days since the epoch, both inclusive: NaN where
    ``start_day <= day < end_day + 1`` for any range, ``day`` the row ``%day`` (R: exclude_dates.py; a NaT day is NaN and in no range)."""
    b = _RowBuilder()
    for col, ranges in excluded.items():
        _numeric(dtypes, col)
        cond = f"%in:{col}"
        for k, (start, end) in enumerate(ranges):
            unit: list[tuple[str, Any, str | None]] = [("copy", DAY_ROW, None)] if k == 0 else []
            first = len(unit)
            unit += [("scalar", b.scalar(float(start)), None), ("cmp_ge", DAY_ROW, None), ("scalar", b.scalar(float(end) + 1.0), None),
                     ("cmp_lt", DAY_ROW, None), ("and", first + 1, None if k else cond)]
            if k:
                unit.append(("or", cond, cond))
            if k == len(ranges) - 1:
                unit.append(("nan_where", col, col))
            b.emit(unit)
    return b.finish(list(excluded))


def compile_clip(ranges: Mapping[str, tuple[Any, Any]], dtypes: Mapping[str, Any]) -> RowProgram:
    """``column -> (low, high)``: ``Series.clip(low, high)`` (R: clip.py) — a NaN bound is no bound, two bounds the wrong way round are
    swapped (both pandas' own), a NaN value stays, ``-0.0`` stays against a bound of 0."""
    b = _RowBuilder()
    results = []
    for col, (low, high) in ranges.items():
        dtype = _numeric(dtypes, col)
        low, high = (None if v is None or v != v else v for v in (low, high))
        if low is not None and high is not None and low > high:
            low, high = high, low
        unit: list[tuple[str, Any, str | None]] = []
        if low is not None:
            unit += [("scalar", b.scalar(round_scalar(low, dtype)), None), ("clip_low", col, None)]
        if high is not None:
            unit += [("scalar", b.scalar(round_scalar(high, dtype)), None), ("clip_high", 1 if unit else col, None)]
        if unit:
            b.emit(unit[:-1] + [(unit[-1][0], unit[-1][1], col)])
            results.append(col)
    return b.finish(results)


def compile_fill_nans(values: Mapping[str, Any], dtypes: Mapping[str, Any]) -> RowProgram:
    """``column -> value``: ``fillna`` of the floating-point columns (R: impute_nans.py)."""
    b = _RowBuilder()
    for col, value in values.items():
        b.emit([("scalar", b.scalar(round_scalar(value, dtypes[col])), None), ("fill_nan", col, col)])
    return b.finish(list(values))


def compile_keep_not_beyond(columns: Sequence[str], threshold: float, dtypes: Mapping[str, Any]) -> RowProgram:
    """``%keep`` = no column has ``|x| > threshold`` (R: remove_extreme_values.py, method ``drop``); a NaN does not exceed it."""
    b = _RowBuilder()
    bad = "%beyond"
    for k, col in enumerate(dict.fromkeys(columns)):
        unit: list[tuple[str, Any, str | None]] = [("scalar", b.scalar(round_scalar(threshold, _numeric(dtypes, col))), None),
                                                    ("abs_gt", col, None if k else bad)]
        b.emit(unit + ([("or", bad, bad)] if k else []))
    b.emit([("not", bad, KEEP_ROW)])
    return b.finish([KEEP_ROW])


def compile_keep_not_missing(columns: Sequence[str], how: str, dtypes: Mapping[str, Any]) -> RowProgram:
    """``%keep`` = not (any / all of the columns are missing) (R: drop_nans.py: ``dropna(how, subset)``).  A floating-point column is
    tested by ``is_nan``; any other enters as the 0 / 1 row ``%missing:<column>`` the caller provides (NaT, None; zeros for integers)."""
    b = _RowBuilder()
    gone = "%gone"
    for k, col in enumerate(dict.fromkeys(columns)):
        test = ("is_nan", col) if _dtype_kind(dtypes[col]) == "f" else ("copy", f"%missing:{col}")
        b.emit([(*test, None if k else gone)] + ([("or" if how == "any" else "and", gone, gone)] if k else []))
    b.emit([("not", gone, KEEP_ROW)])
    return b.finish([KEEP_ROW])


def utc_days(date: Any, dev: torch.device) -> torch.Tensor:
    """``floor(date_ns / 86 400e9)`` as a float64 device row, NaN for NaT: one floor division on the device; the cast is exact."""
    ns = _device(to_ns(date), dev)
    return torch.div(ns, DAY_NS, rounding_mode="floor").to(torch.float64).masked_fill_(ns == NAT, float("nan"))


def row_program(columns: Mapping[str, Any], program: RowProgram, dev: torch.device | None = None,
                rows: Mapping[str, torch.Tensor] | None = None) -> dict[str, torch.Tensor]:
    """``{name: float64 device row}`` of the program's results over the table ``columns`` (a mapping or DataFrame of numpy arrays, pandas
    Series or device tensors) — one launch of ``atx_obs_column_ops`` per ``RowLaunch``.  ``rows``: the ``%`` rows the program reads.  Columns
    are read through ``float_column`` (a float64 device tensor is used in place, anything narrower or integer converts exactly below
    2^53); every result is a fresh row, so the caller's columns are never written.  The scalars go up once, as one float64 tensor."""
    dev = launch_device([*(columns[name] for name in columns.keys()), *(rows or {}).values()], dev)
    scalars = _device(np.asarray(program.scalars, dtype=np.float64), dev) if program.scalars else None
    current: dict[str, torch.Tensor] = {}
    as_float: dict[str, torch.Tensor] = dict(rows or {})

    def row(name: str) -> torch.Tensor:
        if name in current:
            return current[name]
        if name not in as_float:
            as_float[name] = float_column(columns[name], dev)
        return as_float[name]

    for launch in program.launches:
        inputs = [row(slot.read) if slot.read is not None else None for slot in launch.slots]
        lengths = {c.numel() for c in inputs if c is not None}
        if len(lengths) != 1:
            raise ValueError(f"columns differ in length: { {slot.read: c.numel() for slot, c in zip(launch.slots, inputs) if c is not None} }")
        n = lengths.pop()
        outs = [torch.empty(n, dtype=torch.float64, device=dev) if slot.store is not None else None for slot in launch.slots]
        native.obs_column_ops([(native.ROW_OPS[slot.op], slot.src, scalars[slot.scalar:slot.scalar + 1] if slot.op == "scalar" else c, o)
                               for slot, c, o in zip(launch.slots, inputs, outs)], n)
        current.update({slot.store: o for slot, o in zip(launch.slots, outs) if o is not None})
    return {name: current[name] for name in program.results}


def keep_rows(columns: Mapping[str, Any], program: RowProgram, dev: torch.device | None = None,
              rows: Mapping[str, torch.Tensor] | None = None) -> torch.Tensor:
    """The ascending int64 device positions of the rows a keep-row program keeps (its ``%keep`` row is not 0)."""
    return torch.nonzero(row_program(columns, program, dev, rows)[KEEP_ROW]).reshape(-1)


# ---- row expressions: filter_query and mask_values_custom (R: filters/tabular/filter_query.py, mask_values_custom.py) --------------------
ExprProgram = _query.ExprProgram


def compile_query(text: str, dtypes: Mapping[str, Any]) -> ExprProgram:
    """The keep-row program of ``DataFrame.query(text)`` for columns of the dtypes ``dtypes`` (``query.compile_query``: the language, numpy's
    typing and the limits are stated there).  Pure host logic; raises ``ValueError``."""
    return _query.compile_query(text, dtypes)


def _expr_inputs(columns: Mapping[str, Any], program: ExprProgram, dev: torch.device, rows: Mapping[str, torch.Tensor] | None) -> list[torch.Tensor]:
    """The program's input rows: a ``%`` row the caller provides, a string leaf evaluated on the host (0 / 1), a bool column as 0 / 1, any
    other column through ``float_column`` (a float64 device tensor is used in place)."""
    inputs = []
    for name in program.inputs:
        if rows and name in rows:
            inputs.append(rows[name])
        elif name.startswith(_query.HOST_ROW):
            leaf = program.host[int(name[len(_query.HOST_ROW):])]
            inputs.append(_device(_query.host_leaf(leaf, host_array(columns[leaf.column])).astype(np.float64), dev))
        elif _dtype_kind(columns[name].dtype if isinstance(columns[name], torch.Tensor) else host_array(columns[name]).dtype) == "b":
            column = columns[name] if isinstance(columns[name], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(host_array(columns[name])))
            inputs.append(column.reshape(-1).to(device=dev, dtype=torch.float64).contiguous())
        else:
            inputs.append(float_column(columns[name], dev))
    if len({c.numel() for c in inputs}) > 1:
        raise ValueError(f"columns differ in length: { {name: c.numel() for name, c in zip(program.inputs, inputs)} }")
    return inputs


def _expr_code(program: ExprProgram) -> list[tuple[int, int, int]]:
    return [(native.EXPR_OPS[op], a, b) for op, a, b in program.code]


def _n_rows(columns: Mapping[str, Any], inputs: Sequence[torch.Tensor]) -> int:
    if inputs:
        return inputs[0].numel()
    return len(columns) if hasattr(columns, "columns") else next((len(columns[name]) for name in columns.keys()), 0)


def query_rows(columns: Mapping[str, Any], program: ExprProgram, dev: torch.device | None = None,
               rows: Mapping[str, torch.Tensor] | None = None) -> torch.Tensor:
    """The ascending int64 device positions of the rows a keep program keeps: ONE launch of ``native.obs_row_expr`` writes a bit per row and a
    count per chunk of ``native.EXPR_CHUNK_ROWS`` rows, ``torch.cumsum`` scans the counts (its last element, read once on the host,
    sizes the result — the one synchronisation), and ``native.obs_keep_positions`` expands the bits."""
    assert program.keep and not program.results
    dev = launch_device([*(columns[name] for name in columns.keys()), *(rows or {}).values()], dev)
    inputs = _expr_inputs(columns, program, dev, rows)
    n = _n_rows(columns, inputs)
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    words = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
    counts = torch.empty((n + native.EXPR_CHUNK_ROWS - 1) // native.EXPR_CHUNK_ROWS, dtype=torch.int64, device=dev)
    native.obs_row_expr(_expr_code(program), inputs, program.consts, [], n, keep_words=words, chunk_counts=counts)
    ends = torch.cumsum(counts, 0)
    positions = torch.empty(int(ends[-1]), dtype=torch.int64, device=dev)
    native.obs_keep_positions(words, ends - counts, n, positions)
    return positions


def eval_rows(columns: Mapping[str, Any], program: ExprProgram, dev: torch.device | None = None,
              rows: Mapping[str, torch.Tensor] | None = None) -> dict[str, torch.Tensor]:
    """``{name: float64 device row}`` of a program's value results (``query.compile_masks``), one launch; every result is a fresh row."""
    assert program.results and not program.keep
    dev = launch_device([*(columns[name] for name in columns.keys()), *(rows or {}).values()], dev)
    inputs = _expr_inputs(columns, program, dev, rows)
    n = _n_rows(columns, inputs)
    outs = [torch.empty(n, dtype=torch.float64, device=dev) for _ in program.results]
    if n:
        native.obs_row_expr(_expr_code(program), inputs, program.consts, outs, n)
    return dict(zip(program.results, outs))


# ---- station identifiers: encode_statids ----------------------------------------------------------------------------------------------
_BASE36 = frozenset("0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ")


def statid_to_int(station_id: str) -> int:
    """R: filters/tabular/encode_statids.py:45-57 — the base-36 value of the stripped, upper-cased identifier if it is made of 0-9A-Z,
    else the first four bytes of the MD5 digest of the stripped identifier, little-endian.  The host's answer for the rows the kernel
    leaves undecided."""
    import hashlib

    stripped = station_id.strip()
    s = stripped.upper()
    if s and _BASE36.issuperset(s):
        return int(s, 36)
    return int.from_bytes(hashlib.md5(stripped.encode()).digest()[:4], "little", signed=False)


def _int64_codes(values: Sequence[int], what: str) -> np.ndarray:
    beyond = sum(v >= 2**63 for v in values)
    if beyond:
        raise OverflowError(f"encode_statids: {beyond} of {what} encode to 2^63 or more, which no int64 column holds")
    return np.array(values, dtype=np.int64).reshape(-1)


def encode_statids(column: Any, dev: torch.device | None = None, packed: tuple[np.ndarray, int] | None = None) -> tuple[torch.Tensor, int]:
    """``(code, host_rows)``: a column of station identifiers (``str``) as an int64 device row, and how many rows the host decided.
    The column is packed into a byte matrix (``tables.text_matrix``), uploaded and encoded in ONE launch
    (``native_text.encode_statids`` -> ``atx_text_encode_statids``); the rows the kernel flags undecided — non-ASCII, an interior NUL, 13
    or more base-36 characters — are listed (``torch.nonzero``: the one synchronisation), evaluated by ``statid_to_int`` on the
    original strings and scattered in.  A column wider than ``native_text.MAX_WIDTH`` bytes is evaluated on the host as a whole.  A value
    of 2^63 or more raises ``OverflowError``.  ``packed``: what ``text_matrix(column)`` returned, if the caller has it already."""
    from . import native_text
    from .core import say_once
    from .tables import text_matrix

    text, width = packed if packed is not None else text_matrix(column)
    dev = launch_device((), dev)
    strings = host_array(column).reshape(-1)
    n = text.shape[0]
    if width > native_text.MAX_WIDTH:
        say_once(_LOG, "statids-wide", "encode_statids: an identifier of %d bytes is wider than the kernel's %d; the whole column is "
                 "encoded on the host", width, native_text.MAX_WIDTH, level=logging.INFO)
        return _device(_int64_codes([statid_to_int(s) for s in strings.tolist()], f"{n} rows"), dev), n
    code = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return code, 0
    undecided = torch.empty(n, dtype=torch.uint8, device=dev)
    native_text.encode_statids(_device(text, dev)[:, :width], code, undecided)
    rows = torch.nonzero(undecided).reshape(-1)
    if rows.numel():
        values = _int64_codes([statid_to_int(strings[i]) for i in rows.cpu().tolist()], f"{n} rows")
        code[rows] = _device(values, dev)
    return code, rows.numel()
