"""``tables.Table`` and the column readers without a GPU: what a table says of itself, the reference's missing-column message, the
datetime rule, that the caller's table is never returned or modified, the container and column order each kind of table gets back,
the kind letters against numpy's, NaT through every datetime unit — and that none of it looks for the device.

The three kinds of table: a DataFrame, a mapping of numpy arrays, a mapping holding (CPU) tensors, which counts as resident.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from anemoi_transform_amd import native, stack, tables
from anemoi_transform_amd.tables import Table

COLUMNS = {"date": np.array(["2025-01-01T00", "NaT", "2025-01-01T02"], dtype="datetime64[ns]"), "x": np.array([1.5, np.nan, -0.0]),
           "k": np.array([3, 1, 2], dtype=np.int32)}
I64_MIN = np.iinfo(np.int64).min


def _table(kind: str):
    if kind == "frame":
        return pytest.importorskip("pandas").DataFrame(COLUMNS)
    if kind == "tensors":
        return {name: torch.from_numpy(col.view(np.int64) if col.dtype.kind == "M" else col.copy()) for name, col in COLUMNS.items()}
    return {name: col.copy() for name, col in COLUMNS.items()}


KINDS = ["frame", "arrays", "tensors"]


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the device was looked for")

    monkeypatch.setattr(stack, "device", refuse)


@pytest.mark.parametrize("kind", KINDS)
def test_names_rows_and_residency(kind, no_device):
    t = Table(_table(kind))
    assert t.names == ["date", "x", "k"] and t.n_rows == 3
    assert t.frame == (kind == "frame") and t.resident == (kind == "tensors")


def test_tables_without_columns_or_rows(no_device):
    assert Table({}).names == [] and Table({}).n_rows == 0 and not Table({}).resident
    empty = Table({"a": np.zeros(0), "b": torch.zeros(0)})
    assert empty.names == ["a", "b"] and empty.n_rows == 0 and empty.resident
    pd = pytest.importorskip("pandas")
    assert Table(pd.DataFrame()).n_rows == 0 and Table(pd.DataFrame()).names == []
    frame = Table(pd.DataFrame({"a": np.zeros(0)}))
    assert frame.frame and frame.names == ["a"] and frame.n_rows == 0
    with pytest.raises(TypeError, match="a table is a pandas DataFrame or a mapping name -> column, got list"):
        Table([1, 2])


@pytest.mark.parametrize("kind", KINDS)
def test_require_has_the_reference_message(kind, no_device):
    t = Table(_table(kind))
    t.require(["date", "k"])
    t.require([])
    with pytest.raises(ValueError) as e:
        t.require(["k", "col1"])
    assert str(e.value) == "DataFrame is missing columns: {'col1'}. Available columns: ['date', 'x', 'k']"  # R: support/utils.py:18-21


def test_is_datetime():
    ns = torch.from_numpy(COLUMNS["date"].view(np.int64))
    t = Table({"date": ns, "seen": ns, "when": COLUMNS["date"], "secs": COLUMNS["date"].astype("datetime64[s]"), "x": COLUMNS["x"],
               "i": COLUMNS["date"].view(np.int64)})
    assert t.is_datetime("date") and not t.is_datetime("seen")  # an int64 tensor is nanoseconds only under the name `date`
    assert t.is_datetime("when") and t.is_datetime("secs") and not t.is_datetime("x") and not t.is_datetime("i")
    assert not Table({"date": torch.zeros(3)}).is_datetime("date")  # int64, or it is no date
    pd = pytest.importorskip("pandas")
    frame = Table(pd.DataFrame({"when": COLUMNS["date"], "aware": pd.Series(COLUMNS["date"]).dt.tz_localize("UTC"), "x": COLUMNS["x"]}))
    assert frame.is_datetime("when") and frame.is_datetime("aware") and not frame.is_datetime("x")
    # rows taken from a table keep what it said of its columns
    taken = Table({"seen": ns[:2], "date": ns[:2]}, like=t)
    assert not taken.is_datetime("seen") and taken.is_datetime("date")
    was = Table({"when": ns[:2]}, like=t)
    assert was.is_datetime("when") and was.resident


@pytest.mark.parametrize("kind", KINDS)
def test_without_hands_back_the_callers_columns(kind, no_device):
    table = _table(kind)
    out = Table(table).without(["x"])
    assert out is not table and list(out if kind != "frame" else out.columns) == ["date", "k"]
    assert list(table if kind != "frame" else table.columns) == ["date", "x", "k"]
    if kind != "frame":
        assert type(out) is dict and out["date"] is table["date"] and out["k"] is table["k"]


@pytest.mark.parametrize("kind", KINDS)
def test_with_columns_gives_a_new_table_of_the_same_kind(kind, no_device):
    table = _table(kind)
    before = {name: np.array(tables.host_array(table[name])) for name in COLUMNS}
    added = {"x": torch.tensor([7.0, 8.0, 9.0], dtype=torch.float64), "new": torch.tensor([1, 2, 3]),
             "seen": torch.tensor([5, I64_MIN, 6])}
    out = Table(table).with_columns(added, datetimes=["seen"])
    assert out is not table
    assert list(table if kind != "frame" else table.columns) == ["date", "x", "k"]
    assert all(np.array_equal(tables.host_array(table[name]), before[name], equal_nan=True) for name in COLUMNS)
    assert list(out if kind != "frame" else out.columns) == ["date", "x", "k", "new", "seen"]  # replaced in place, new ones appended
    if kind == "frame":
        assert type(out) is type(table) and out["x"].tolist() == [7.0, 8.0, 9.0] and out["new"].dtype == np.int64
        assert out["seen"].dtype == np.dtype("datetime64[ns]") and out["seen"].isna().tolist() == [False, True, False]
    elif kind == "tensors":
        assert type(out) is dict and all(out[name] is added[name] for name in added) and out["k"] is table["k"]
    else:
        assert type(out) is dict and all(isinstance(out[name], np.ndarray) for name in out) and out["k"] is table["k"]
        assert out["x"].tolist() == [7.0, 8.0, 9.0] and out["seen"].dtype == np.dtype("datetime64[ns]") and np.isnat(out["seen"][1])
        assert out["seen"].view(np.int64).tolist() == [5, I64_MIN, 6]


@pytest.mark.parametrize("kind", KINDS)
def test_replaced_overwrites_and_renames_in_place(kind, no_device):
    table = _table(kind)
    before = {name: np.array(tables.host_array(table[name])) for name in COLUMNS}
    out = Table(table).replaced({"x": torch.tensor([7.0, 8.0, 9.0], dtype=torch.float64)}, renamed={"x": "y"})
    assert out is not table and list(out if kind != "frame" else out.columns) == ["date", "y", "k"]
    assert list(table if kind != "frame" else table.columns) == ["date", "x", "k"]
    assert all(np.array_equal(tables.host_array(table[name]), before[name], equal_nan=True) for name in COLUMNS)
    assert tables.host_array(out["y"]).tolist() == [7.0, 8.0, 9.0]
    if kind == "frame":
        assert type(out) is type(table)
    else:
        assert type(out) is dict and isinstance(out["y"], torch.Tensor if kind == "tensors" else np.ndarray) and out["k"] is table["k"]
    same = Table(table).replaced({})
    assert same is not table and list(same if kind != "frame" else same.columns) == ["date", "x", "k"]


def test_take_on_host_tables_is_numpy_and_iloc(no_device):
    rows = torch.tensor([2, 0, 0])
    out = Table(_table("arrays")).take(rows)
    assert list(out) == ["date", "x", "k"] and all(isinstance(v, np.ndarray) for v in out.values())
    assert out["k"].tolist() == [2, 3, 3] and out["k"].dtype == np.int32 and out["date"].dtype == COLUMNS["date"].dtype
    assert list(Table(_table("arrays")).take(rows, names=["k", "x"])) == ["k", "x"]
    pd = pytest.importorskip("pandas")
    frame = pd.DataFrame(COLUMNS, index=["a", "b", "c"])
    out = Table(frame).take(rows)
    assert out.index.tolist() == ["c", "a", "a"] and out.equals(frame.iloc[[2, 0, 0]])  # the rows travel with their labels
    part = Table(frame).take(rows, names=["k"])
    assert list(part.columns) == ["k"] and part.index.tolist() == ["c", "a", "a"] and part["k"].tolist() == [2, 3, 3]
    assert len(Table(frame).take(rows, names=[])) == 3


KIND_DTYPES = [*native.KEY_DTYPES, torch.float16, torch.uint16, torch.uint32, torch.uint64, torch.complex64]


@pytest.mark.parametrize("dtype", KIND_DTYPES, ids=str)
def test_kind_letters_are_numpys(dtype):
    as_numpy = torch.zeros(2, dtype=dtype).numpy().dtype
    assert tables.dtype_kind(dtype) == tables.dtype_kind(as_numpy) == as_numpy.kind
    assert tables.column_kind(torch.zeros(2, dtype=dtype)) == tables.column_kind(np.zeros(2, dtype=as_numpy)) == as_numpy.kind


def test_kind_letters_of_datetimes_and_objects():
    assert {torch.float64, torch.float32, torch.int64, torch.int8, torch.uint8, torch.bool} <= set(native.KEY_DTYPES)
    assert tables.dtype_kind(np.dtype("datetime64[s]")) == "M" == tables.column_kind(COLUMNS["date"].astype("datetime64[s]"))
    assert tables.column_kind(np.zeros(2, dtype="timedelta64[ms]")) == "m"
    assert tables.dtype_kind(np.dtype(object)) == "O" == tables.column_kind(np.array(["a", None], dtype=object))
    assert tables.dtype_kind(np.dtype("U3")) == "U" and tables.column_kind(np.array(["abc"])) == "O"  # not numeric: one letter for all
    assert tables.column_kind(["a", "b"]) == "O" and tables.column_kind([1.0, 2.0]) == "f"
    pd = pytest.importorskip("pandas")
    assert tables.column_kind(pd.Series(COLUMNS["date"]).dt.tz_localize("UTC")) == "M"
    assert tables.column_kind(pd.Series(["a", "b"], dtype="category")) == "O" and tables.column_kind(pd.Series([1, 2])) == "i"


def test_datetime_ns_is_the_same_through_every_unit():
    ns = COLUMNS["date"]
    want = ns.view(np.int64)
    assert want[1] == I64_MIN == tables.NAT
    for unit in ("s", "ms", "ns"):
        got = tables.datetime_ns(ns.astype(f"datetime64[{unit}]"))
        assert got.dtype == np.int64 and got.flags.c_contiguous and np.array_equal(got, want), unit
        assert np.array_equal(tables.to_ns(ns.astype(f"datetime64[{unit}]")), want)
    assert tables.datetime_ns(np.array([1, "NaT"], dtype="timedelta64[s]")).tolist() == [10**9, I64_MIN]
    assert tables.datetime_ns(ns.reshape(3, 1)[::-1]).tolist() == want[::-1].tolist()  # any shape and stride: one contiguous row
    # to_ns: int64 IS nanoseconds, array or tensor; any other tensor is refused
    assert tables.to_ns(want).tolist() == want.tolist() and tables.to_ns(torch.from_numpy(want)).tolist() == want.tolist()
    assert tables.to_ns(["2025-01-01T00:00:00", "NaT", "2025-01-01T02:00:00"]).tolist() == want.tolist()
    with pytest.raises(ValueError, match="int64 nanoseconds"):
        tables.to_ns(torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="cannot read a date column of dtype <U9 as datetimes"):
        tables.to_ns(np.array(["yesterday"]))


def test_float_column_refuses_bool_and_complex():
    cpu = torch.device("cpu")
    for bad in (np.array([True]), np.array([1j]), torch.tensor([True]), torch.tensor([1j]), np.array(["a"])):
        with pytest.raises(ValueError, match="a numeric column is needed"):
            tables.float_column(bad, cpu)
    got = tables.float_column(np.array([1, 2], dtype=np.uint16), cpu)
    assert got.dtype == torch.float64 and got.tolist() == [1.0, 2.0]
    assert tables.float_column(torch.tensor([1.5], dtype=torch.float16), cpu).tolist() == [1.5]


@pytest.mark.parametrize("kind", KINDS)
def test_the_device_is_looked_for_on_first_use_only(kind, no_device):
    t = Table(_table(kind))
    t.require(["x"])
    assert t.names and t.n_rows == 3 and t.without(["k"]) is not None and t.is_datetime("date")
    with pytest.raises(AssertionError, match="the device was looked for"):
        t.device
