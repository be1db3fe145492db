"""One observation table, read once: what its columns are, where a launch over them runs and what goes back to the caller.

A table is a pandas DataFrame or a plain mapping ``name -> 1-D column``; a column is a numpy array, a pandas Series, a list or a
torch tensor.  The first half are the column readers every tabular routine shares (``host_array``, ``column_kind``, ``datetime_ns``,
``to_ns``, ``float_column``, ``on_device``, ``launch_device``), ``text_matrix`` — what a column of strings is to a text kernel: a
zero-padded byte matrix — and the one gather of many columns by one row list (``take_rows`` -> ``atx_obs_take_rows``).  The second half is ``Table``, which every tabular filter wraps its argument in.  The rules it states once:

  * the launch runs where the table's first CUDA tensor lives, else on this process's device (``stack.device()``) — looked up on
    first use, so a filter that raises a host error first never touches the device;
  * a DataFrame gives a DataFrame; a mapping gives a new dict, of device tensors if any input column was a tensor (``resident``),
    else of numpy arrays; the caller's object is never returned or modified (``without`` alone hands back the caller's columns);
  * datetimes are int64 nanoseconds on the device (NaT = ``INT64_MIN``): a datetime64 column says so itself, an int64 tensor named
    ``date`` IS nanoseconds;
  * a non-numeric host column cannot live on the device and stays a host array, also in a resident table;
  * DataFrame rows are taken with ``iloc``: they travel with their index labels.
"""

from __future__ import annotations

import sys
from collections.abc import Mapping
from typing import Any, Iterable, Sequence

import numpy as np
import torch

from . import native
from . import stack as _stack

NAT = np.iinfo(np.int64).min  # numpy's / pandas' NaT as int64


# ---- column readers ---------------------------------------------------------------------------------------------------------------------
def host_array(column: Any) -> np.ndarray:
    """The column as a numpy array on the host: a tz-aware pandas Series as naive UTC, a device tensor copied down."""
    if isinstance(column, torch.Tensor):
        return column.cpu().numpy()
    if hasattr(column, "dt") and getattr(column.dt, "tz", None) is not None:  # a tz-aware pandas Series: all times are UTC
        column = column.dt.tz_convert(None)
    if hasattr(column, "to_numpy"):
        return column.to_numpy()
    return np.asarray(column)


def dtype_kind(dtype: Any) -> str:
    """numpy's kind letter of a numpy or torch dtype: b, i, u, f, c — anything else is not numeric."""
    if isinstance(dtype, torch.dtype):
        if dtype == torch.bool:
            return "b"
        if dtype.is_complex:
            return "c"
        return "f" if dtype.is_floating_point else ("u" if str(dtype).startswith("torch.uint") else "i")  # uint8, uint16, uint32, uint64
    return np.dtype(dtype).kind


def column_kind(column: Any) -> str:
    """numpy's kind letter of a tensor, an array or a Series alike — b, i, u, f, c, M, m — and ``"O"`` for anything not numeric."""
    kind = dtype_kind(column.dtype if isinstance(column, torch.Tensor) else host_array(column).dtype)
    return kind if kind in "biufcMm" else "O"


def datetime_ns(a: np.ndarray) -> np.ndarray:
    """A datetime64 or timedelta64 array of any unit as contiguous int64 nanoseconds, NaT = ``INT64_MIN``."""
    unit = "timedelta64[ns]" if a.dtype.kind == "m" else "datetime64[ns]"
    return np.ascontiguousarray(a.astype(unit).reshape(-1)).view(np.int64)


def to_ns(column: Any) -> np.ndarray | torch.Tensor:
    """A column of datetimes as int64 nanoseconds since the epoch, NaT = ``INT64_MIN``.  datetime64 arrays of any unit, pandas
    Series, lists of datetimes or ISO strings; an int64 array or tensor is taken to BE nanoseconds already."""
    if isinstance(column, torch.Tensor):
        if column.dtype != torch.int64:
            raise ValueError(f"a date tensor must hold int64 nanoseconds, got {column.dtype}")
        return column.reshape(-1)
    a = host_array(column)
    if a.dtype.kind == "i":
        return np.ascontiguousarray(a.reshape(-1), dtype=np.int64)
    try:
        return datetime_ns(a if a.dtype.kind == "M" else a.astype("datetime64[ns]"))
    except (ValueError, TypeError) as e:
        raise ValueError(f"cannot read a date column of dtype {a.dtype} as datetimes: {e}") from None


def on_device(x: np.ndarray | torch.Tensor, dev: torch.device) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return t.to(dev).contiguous()


def launch_device(columns: Iterable[Any], dev: torch.device | None = None) -> torch.device:
    """Where a launch over ``columns`` runs: ``dev`` if given, else where the first CUDA tensor among them lives, else this
    process's device."""
    if dev is not None:
        return dev
    return next((c.device for c in columns if isinstance(c, torch.Tensor) and c.is_cuda), None) or _stack.device()


def float_column(column: Any, dev: torch.device) -> torch.Tensor:
    """A numeric column as a contiguous float64 device row (a device tensor is used in place when it already is one)."""
    if isinstance(column, torch.Tensor):
        if column_kind(column) in "bc":
            raise ValueError(f"a numeric column is needed, got {column.dtype}")
        return column.reshape(-1).to(device=dev, dtype=torch.float64).contiguous()
    a = host_array(column)
    if column_kind(a) not in "iuf":
        raise ValueError(f"a numeric column is needed, got dtype {a.dtype}")
    return on_device(np.ascontiguousarray(a.reshape(-1), dtype=np.float64), dev)


def text_matrix(column: Any) -> tuple[np.ndarray, int]:
    """A column of ``str`` as the byte matrix the text kernels read (``include/atx_text.h``): uint8 ``[n, pitch]``, row ``r`` the bytes of
    its string zero-padded to ``width`` (the longest string, at least 1), ``pitch`` the next multiple of 4.  Returns ``(matrix, width)``.
    A pandas Series, an object array or a numpy ``U`` array.  The bytes are the code points themselves, which is UTF-8 for ASCII; a row
    with a code point above 127 gets a first byte of 0x80, so that the kernel's own rule for such bytes hands the row to the host — its
    other bytes mean nothing.  Anything in the column that is not a ``str`` (None, NaN, ``pd.NA``, a number, ``bytes``, an ``S`` array,
    a tensor) raises ``ValueError`` with the count: numpy's own conversion would turn ``None`` into ``'None'``.  A ``U`` array is read
    with vectorised numpy only; an object column goes through numpy's conversion to ``U`` once, which drops trailing U+0000."""
    if isinstance(column, torch.Tensor):
        raise ValueError(f"a text column holds str, got a {column.dtype} tensor")
    a = host_array(column).reshape(-1)
    if a.dtype.kind == "O":
        not_str = sum(not isinstance(v, str) for v in a.tolist())
        if not_str:
            raise ValueError(f"a text column holds str: {not_str} of {a.size} entries are something else (None, NaN, a number, bytes)")
        a = a.astype("U") if a.size else np.zeros(0, dtype="U1")
    elif a.dtype.kind != "U":
        raise ValueError(f"a text column holds str: {a.size} of {a.size} entries are of dtype {a.dtype}")
    chars = a.dtype.itemsize // 4
    points = np.ascontiguousarray(a.astype(a.dtype.newbyteorder("="), copy=False)).view(np.uint32).reshape(a.size, chars)
    width = max(chars, 1)
    matrix = np.zeros((a.size, (width + 3) // 4 * 4), dtype=np.uint8)
    matrix[:, :chars] = points  # narrowed modulo 256: exact for ASCII
    matrix[(points > 127).any(axis=1), 0] = 0x80
    return matrix, width


def gather(columns: Sequence[torch.Tensor], rows: torch.Tensor, check: bool = True) -> list[torch.Tensor]:
    """``[c[rows] for c in columns]`` for contiguous device rows of equal length: one launch of ``atx_obs_take_rows`` per 16 columns."""
    columns = list(columns)
    step = native.MAX_ROWSET_COLUMNS
    outs = [torch.empty(rows.numel(), dtype=c.dtype, device=rows.device) for c in columns]
    n_bad = torch.zeros(max((len(columns) + step - 1) // step, 1), dtype=torch.int64, device=rows.device)
    for j in range(0, len(columns), step):
        native.obs_take_rows(columns[j:j + step], outs[j:j + step], rows, n_bad[j // step:j // step + 1])
    if check and columns and rows.numel():
        bad = int(n_bad[0])  # every launch of the call sees the same rows
        if bad:
            raise IndexError(f"take_rows: {bad} of {rows.numel()} row indices lie outside the table's {columns[0].numel()} rows")
    return outs


def take_rows(columns: Mapping[str, Any], rows: Any, dev: torch.device | None = None) -> dict[str, torch.Tensor]:
    """``{name: column[rows]}`` as device tensors — one launch of ``atx_obs_take_rows`` per 16 columns, the row list read once per row
    for all of them.  Dtypes are kept (anything of 1, 2, 4 or 8 bytes per element); datetime64 columns come back as int64
    nanoseconds.  numpy columns are uploaded, device tensors used in place; ``rows``: int64 positions, array or tensor, in any order and
    with repeats.  A position outside the table raises ``IndexError`` with the count (synchronises; the kernel reads nothing through it)."""
    dev = launch_device((*columns.values(), rows), dev)
    rows = on_device(rows if isinstance(rows, torch.Tensor) else np.asarray(rows, dtype=np.int64), dev).reshape(-1)
    if rows.dtype != torch.int64:
        raise ValueError(f"row positions must be int64, got {rows.dtype}")
    cols = {}
    for name, col in columns.items():
        if not isinstance(col, torch.Tensor):
            a = host_array(col).reshape(-1)
            if column_kind(a) in "Mm":
                a = datetime_ns(a)
            elif column_kind(a) not in "iufbc":
                raise ValueError(f"column {name!r} of dtype {a.dtype} cannot live on the device")
            col = torch.from_numpy(np.ascontiguousarray(a))
        if col.element_size() not in (1, 2, 4, 8):
            raise ValueError(f"column {name!r}: elements of {col.element_size()} bytes (1, 2, 4 or 8 are taken)")
        cols[name] = col.reshape(-1).to(dev).contiguous()
    if len({c.numel() for c in cols.values()}) > 1:
        raise ValueError(f"columns differ in length: { {name: c.numel() for name, c in cols.items()} }")
    return dict(zip(cols, gather(list(cols.values()), rows)))


# ---- the table --------------------------------------------------------------------------------------------------------------------------
class Table:
    """One input table of a tabular filter: a pandas DataFrame or a ``Mapping`` name -> column, anything else raises ``TypeError``.
    ``names``: the columns in order; ``n_rows``; ``frame``: it is a DataFrame; ``resident``: some column is a ``torch.Tensor``;
    ``device``: where the launches run (``launch_device`` of the columns, looked up on first use).  ``like``: the table this one was
    made of, by taking rows or columns: it answers ``resident``, ``device`` and ``is_datetime`` as that one does — a datetime64 host
    column of a resident table is an int64 tensor once its rows were taken, and a table may lose its last tensor with a column."""

    def __init__(self, table: Any, like: "Table | None" = None) -> None:
        pd = sys.modules.get("pandas")  # a table can only be a DataFrame if the caller has imported pandas
        self.table = table
        self.frame = pd is not None and isinstance(table, pd.DataFrame)
        if self.frame:
            self.names = list(table.columns)
        elif isinstance(table, Mapping):
            self.names = list(table.keys())
        else:
            raise TypeError(f"a table is a pandas DataFrame or a mapping name -> column, got {type(table).__name__}")
        self.n_rows = len(table) if self.frame else (len(table[self.names[0]]) if self.names else 0)
        self.resident = like.resident if like else not self.frame and any(isinstance(table[name], torch.Tensor) for name in self.names)
        self.datetimes = {name for name in like.names if like.is_datetime(name)} if like else set()
        self._device: torch.device | None = like._device if like else None

    @property
    def device(self) -> torch.device:
        if self._device is None:
            self._device = launch_device(() if self.frame else (self.table[name] for name in self.names))
        return self._device

    def __getitem__(self, name: str) -> Any:
        return self.table[name]

    def require(self, names: Sequence[str]) -> None:
        # R: filters/tabular/support/utils.py:18-21
        missing = set(names) - set(self.names)
        if missing:
            raise ValueError(f"DataFrame is missing columns: {missing}. Available columns: {self.names}")

    def is_datetime(self, name: str) -> bool:
        """datetime64 says so itself; an int64 device tensor named ``date`` is nanoseconds (``to_ns``)."""
        column = self[name]
        if isinstance(column, torch.Tensor):
            return column.dtype == torch.int64 and (name == "date" or name in self.datetimes)
        return column_kind(column) == "M"

    def _host(self, column: torch.Tensor, name: str, datetimes: Iterable[str]) -> np.ndarray:
        a = column.cpu().numpy()
        return a.view("datetime64[ns]") if name in datetimes else a

    def with_columns(self, added: Mapping[str, torch.Tensor], datetimes: Iterable[str] = ()) -> Any:
        """The table with the device rows ``added`` (an existing name keeps its place, a new one goes to the end): ``DataFrame.assign``
        with host arrays for a DataFrame; for a mapping a new dict, the rows as they are if ``resident``, else as numpy arrays.  The
        names in ``datetimes`` are int64 nanoseconds: datetime64[ns] wherever they come to the host."""
        if self.frame:
            return self.table.assign(**{name: self._host(col, name, datetimes) for name, col in added.items()})
        return {**self.table, **{name: (col if self.resident else self._host(col, name, datetimes)) for name, col in added.items()}}

    def replaced(self, columns: Mapping[str, torch.Tensor], renamed: Mapping[str, str] | None = None) -> Any:
        """The table with the columns ``columns`` overwritten by device rows and then renamed by ``renamed``, in place in the column
        order: ``copy()``, assignment and ``rename`` for a DataFrame, a new dict otherwise (device rows if ``resident``, else numpy)."""
        renamed = renamed or {}
        if self.frame:
            out = self.table.copy()
            for name, col in columns.items():
                out[name] = col.cpu().numpy()
            return out.rename(columns=renamed)
        return {renamed.get(name, name): ((columns[name] if self.resident else columns[name].cpu().numpy()) if name in columns else self[name])
                for name in self.names}

    def without(self, names: Sequence[str]) -> Any:
        """The table without the columns ``names``: pandas' ``drop`` for a DataFrame, otherwise a new dict of the caller's own column
        objects — nothing is copied."""
        if self.frame:
            return self.table.drop(labels=list(names), axis=1)
        gone = set(names)
        return {name: self[name] for name in self.names if name not in gone}

    def take(self, rows: torch.Tensor, names: Sequence[str] | None = None) -> Any:
        """The rows at the device positions ``rows`` of the columns ``names`` (default: all), never the caller's object: ``iloc`` for a
        DataFrame (index labels and dtypes are pandas' own); for a resident mapping ONE ``take_rows`` over every column that can live
        on the device and host indexing for the rest; for a host mapping numpy indexing."""
        if self.frame:
            return self.table.iloc[host_array(rows)] if names is None else self.table.iloc[host_array(rows), [self.names.index(n) for n in names]]
        names = self.names if names is None else list(names)
        taken: dict[str, Any] = {}
        if self.resident:
            taken = take_rows({name: self[name] for name in names if column_kind(self[name]) != "O"}, rows, dev=self.device)
        if len(taken) < len(names):
            host = host_array(rows)
            taken.update({name: np.asarray(host_array(self[name]))[host] for name in names if name not in taken})
        return {name: taken[name] for name in names}

    # ---- what superob alone needs of a column --------------------------------------------------------------------------------------
    def missing(self, name: str, dev: torch.device) -> torch.Tensor:
        """Where the column has no value (NaN / NaT / None), a bool row on the device."""
        column = self[name]
        if self.is_datetime(name):
            return on_device(to_ns(column), dev) == NAT
        kind = column_kind(column)
        if kind in "iub":
            return torch.zeros(len(column), dtype=torch.bool, device=dev)
        if isinstance(column, torch.Tensor):
            return torch.isnan(column.reshape(-1)).to(dev)
        a = host_array(column)
        return on_device(np.isnan(a) if kind == "f" else np.array([v is None or v != v for v in a.tolist()], dtype=bool), dev)

    def as_float64(self, name: str, out: torch.Tensor) -> None:
        """The column as float64 into the device row ``out``: integers and bools converted, datetimes as ``(double)`` of their int64
        nanoseconds with NaT as NaN — what pandas hands to its group mean.  Anything else cannot be averaged: ``TypeError``."""
        column = self[name]
        if self.is_datetime(name):
            ns = on_device(to_ns(column), out.device)
            out.copy_(ns)
            out.masked_fill_(ns == NAT, float("nan"))
            return
        if not isinstance(column, torch.Tensor):
            a = host_array(column)
            if column_kind(a) not in "iubf":
                raise TypeError(f"superob: column {name!r} of dtype {a.dtype} cannot be averaged; name it in columns_to_groupby or "
                                "columns_to_take_nearest, or drop it first")
            column = torch.from_numpy(np.ascontiguousarray(a.reshape(-1)))
        elif column.dtype.is_complex:
            raise TypeError(f"superob: column {name!r} of dtype {column.dtype} cannot be averaged")
        out.copy_(column.reshape(-1))
