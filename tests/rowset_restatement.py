"""``sort_by`` and ``drop_duplicates`` in plain numpy: the order key of a value ON ITS BIT PATTERN, the lexicographic stable order of a
tuple of keys, the first occurrences — and the seeded tables that the recorder, the host test and the GPU test share.

The statement (R: filters/tabular/sort_by.py:51 ``df.sort_values(by=columns, kind="stable")``, drop_duplicates.py:61
``df.drop_duplicates(subset)``) is pandas' order and equality, not IEEE's: ``-0.0`` and ``0.0`` are one key, every NaN is one key and
the last, NaT likewise, +-inf order as numbers, int64 compares as integers.  tests/test_rowset_host.py holds this file to pandas
itself on the seeded tables; tests/test_gpu_rowset.py holds the kernels to this file.
"""

from __future__ import annotations

import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowset.json")
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
INF_BITS = 0x7FF0000000000000
GRID_CAP_ROWS = 2048 * 256  # kRsGrid workgroups of 256 lanes: past it a lane takes a second row
# the dtype codes of atx_obs_order_key (atx_key_dtype), by numpy dtype
CODES = {"float64": 0, "float32": 1, "int64": 2, "int32": 3, "int16": 4, "int8": 5, "uint8": 6, "bool": 7, "datetime": 8}


# ---- the key map ---------------------------------------------------------------------------------------------------------------------------
def float_key(x: np.ndarray) -> np.ndarray:
    """float64 / float32 values to int64 keys, on the bits.  float32 is widened first (exact).  With m the magnitude bits: NaN (m above
    infinity's pattern) -> INT64_MAX; a set sign bit -> -m (so -0.0 -> 0, the key of 0.0); else the pattern itself."""
    with np.errstate(invalid="ignore"):  # widening a signalling float32 NaN quiets it, with a warning
        b = np.ascontiguousarray(np.asarray(x).astype(np.float64)).view(np.int64)
    m = b & I64_MAX
    with np.errstate(over="ignore"):
        return np.where(m > INF_BITS, I64_MAX, np.where(b >= 0, b, -m))


def order_key(column: np.ndarray, datetime: bool = False) -> np.ndarray:
    """The int64 key of every entry of a numeric, bool or datetime column (``datetime``: int64 nanoseconds, NaT = INT64_MIN)."""
    a = np.asarray(column)
    if a.dtype.kind == "M":
        a, datetime = a.astype("datetime64[ns]").view(np.int64), True
    if datetime:
        assert a.dtype == np.int64
        return np.where(a == I64_MIN, I64_MAX, a)
    if a.dtype.kind == "f":
        return float_key(a)
    if a.dtype.kind == "b":
        return (a.view(np.uint8) != 0).astype(np.int64)
    assert a.dtype.kind in "iu" and not (a.dtype.kind == "u" and a.dtype.itemsize == 8), a.dtype
    return a.astype(np.int64)


def string_ranks(column) -> np.ndarray:
    """Strings (``None`` for missing) to int64 ranks by Python's own ``sorted``, missing last — independent of pandas' factorize."""
    values = list(column)
    present = sorted({v for v in values if v is not None})
    rank = {v: r for r, v in enumerate(present)}
    return np.array([len(present) if v is None else rank[v] for v in values], dtype=np.int64)


def table_keys(table: dict, names) -> list[np.ndarray]:
    return [string_ranks(table[n]) if np.asarray(table[n]).dtype.kind in "OUS" else order_key(table[n]) for n in names]


# ---- order and first occurrences ------------------------------------------------------------------------------------------------------------
def stable_order(keys) -> np.ndarray:
    """Positions of the rows in ascending order of the key tuple (first key most significant), equal tuples in table order — an
    insertion of every row into Python's own stable ``sorted`` for small tables, ``np.lexsort`` (stable by definition) for large ones."""
    keys = [np.asarray(k, dtype=np.int64) for k in keys]
    n = keys[0].size
    if n <= 4096:
        tuples = list(zip(*[k.tolist() for k in keys]))
        return np.array(sorted(range(n), key=tuples.__getitem__), dtype=np.int64)
    return np.lexsort(keys[::-1]).astype(np.int64)


def first_occurrences(keys) -> np.ndarray:
    """Ascending positions of the first row of every distinct key tuple — a dict of seen tuples for small tables, adjacent
    differences in ``stable_order`` for large ones."""
    keys = [np.asarray(k, dtype=np.int64) for k in keys]
    n = keys[0].size
    if n <= 4096:
        seen, rows = set(), []
        for i, t in enumerate(zip(*[k.tolist() for k in keys])):
            if t not in seen:
                seen.add(t)
                rows.append(i)
        return np.array(rows, dtype=np.int64)
    return np.nonzero(mark_first(keys, stable_order(keys)))[0].astype(np.int64)


def mark_first(keys, order, keep: np.ndarray | None = None) -> np.ndarray:
    """``atx_obs_mark_first`` restated: keep[order[i]] = (i == 0) or any key differs between order[i] and order[i - 1]; with a ``keep``
    given, OR-ed into it."""
    keys = [np.asarray(k, dtype=np.int64) for k in keys]
    order = np.asarray(order, dtype=np.int64)
    differs = np.ones(order.size, dtype=bool)
    if order.size > 1:
        differs[1:] = np.logical_or.reduce([k[order[1:]] != k[order[:-1]] for k in keys])
    out = np.zeros(order.size, dtype=np.uint8) if keep is None else keep.copy()
    out[order] = differs.astype(np.uint8) if keep is None else (out[order] | differs.astype(np.uint8))
    return out


# ---- values that the kernels can get wrong --------------------------------------------------------------------------------------------------
def f64(bits: int) -> float:
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


NAN_POS, NAN_NEG, NAN_PAYLOAD, NAN_SIGNALLING = f64(0x7FF8000000000000), f64(0xFFF8000000000000), f64(0x7FF80000DEADBEEF), f64(0xFFF0000000000001)
F64_POOL = np.array([0.0, -0.0, NAN_POS, NAN_NEG, NAN_PAYLOAD, NAN_SIGNALLING, np.inf, -np.inf, 1.5, -1.5, 5e-324, -5e-324, 2.2250738585072014e-308,
                     -2.2250738585072014e-308, 1e300, -1e300, 2.0, 1.0000000000000002, 1.0])
F32_POOL = np.array([0x00000000, 0x80000000, 0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFF800001, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001,
                     0x40500000, 0xC0500000, 0x3F800001, 0x3F800000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32).view(np.float32)
I64_POOL = np.array([2**53, 2**53 + 1, I64_MIN, I64_MAX, 0, -1, 7, 2**53 - 1, -(2**53) - 1, -(2**53)], dtype=np.int64)
DATE_POOL = np.array(["NaT", "1969-12-31T23:59:59.999999999", "1960-01-01", "1970-01-01", "2020-02-29T12:00", "2020-02-29T12:00:00.000000001",
                      "1677-09-21T00:12:43.145224193", "2262-04-11T23:47:16.854775806"], dtype="datetime64[ns]")  # the last: one below pandas' Timestamp.max, whose int64 is the NaT key
NAME_POOL = ["b", "a", "ab", "", "B", None, "synop", "a "]


def key_specials(code: str) -> np.ndarray:
    """Every special of one dtype code, for the kernel test of ``atx_obs_order_key``."""
    if code == "float64":
        rng = np.random.default_rng(11)
        return np.concatenate([F64_POOL, rng.integers(0, 2**64, 200, dtype=np.uint64).view(np.float64), rng.normal(0, 1e3, 100)])
    if code == "float32":
        rng = np.random.default_rng(12)
        return np.concatenate([F32_POOL, rng.integers(0, 2**32, 200, dtype=np.uint32).view(np.float32), rng.normal(0, 1e3, 100).astype(np.float32)])
    if code == "int64":
        return np.concatenate([I64_POOL, np.random.default_rng(13).integers(I64_MIN, I64_MAX, 200, dtype=np.int64)])
    if code == "datetime":
        return np.concatenate([DATE_POOL.view(np.int64), np.random.default_rng(14).integers(-(2**62), 2**62, 200, dtype=np.int64)])
    if code == "bool":
        return np.random.default_rng(15).random(300) < 0.5
    info = np.iinfo(code)
    return np.concatenate([np.array([info.min, info.max, 0, 1], dtype=code),
                           np.random.default_rng(16).integers(info.min, int(info.max) + 1, 300).astype(code)])


# ---- the seeded tables -----------------------------------------------------------------------------------------------------------------------
SEEDED_ROWS = (48, 300)
SORT_CASES = (["key_f"], ["date"], ["key_k"], ["name"], ["key_g", "key_b"], ["key_b", "date", "key_f"], ["key_k", "name", "key_g"])
DEDUP_CASES = (dict(columns=["key_f"]), dict(columns=["date", "key_k"]), dict(columns=["name", "key_b"]), dict(column_prefix="key_"),
               dict(only=["key_f", "key_b", "name"]))  # the last: no subset, on a table of those three columns alone


def seeded_table(n: int) -> dict:
    """A table of ``n`` rows whose key columns are drawn from the small pools above.  Three rows in four copy ALL their keys from one of
    a few prototype rows, so that whole tuples repeat whatever the subset; the first rows of every column run through its pool, so
    that every special is there; one permutation then shuffles the rows.  ``value`` (int32) is distinct per row; ``label`` holds the
    DataFrame's index labels, which are not 0 .. n - 1."""
    rng = np.random.default_rng(7000 + n)
    pools = {"key_f": F64_POOL, "key_g": F32_POOL, "key_k": I64_POOL, "key_b": np.array([False, True]), "date": DATE_POOL, "name": NAME_POOL}
    n_proto = max(4, n // 8)
    proto_of = np.where(rng.random(n) < 0.75, rng.integers(0, n_proto, n), -1)
    shuffle = rng.permutation(n)
    table = {}
    for column, pool in pools.items():
        proto = rng.integers(0, len(pool), n_proto)
        idx = np.where(proto_of >= 0, proto[proto_of], rng.integers(0, len(pool), n))
        idx[:len(pool)] = np.arange(len(pool))
        idx = idx[shuffle]
        if column == "name":
            table[column] = np.empty(n, dtype=object)
            table[column][:] = [pool[i] for i in idx]
        else:
            table[column] = pool[idx]
    table["value"] = rng.permutation(n).astype(np.int32)
    table["label"] = (100 + 3 * rng.permutation(n)).astype(np.int64)
    return table


def seeded_cases() -> list[dict]:
    """``{"id", "filter", "config", "rows", "columns"}``: the filter to build, the seeded table (by its row count) and the columns of
    it that make up the table the filter sees."""
    out = []
    for n in SEEDED_ROWS:
        everything = [c for c in seeded_table(n) if c != "label"]
        for columns in SORT_CASES:
            out.append(dict(id=f"seeded_{n}_sort_by_{'_'.join(columns)}", filter="sort_by", config=dict(columns=list(columns)), rows=n,
                            columns=everything))
        for spec in DEDUP_CASES:
            config = {k: v for k, v in spec.items() if k != "only"}
            tag = "all_columns" if "only" in spec else ("_".join(spec["columns"]) if "columns" in spec else "prefix_" + spec["column_prefix"])
            out.append(dict(id=f"seeded_{n}_drop_duplicates_{tag}", filter="drop_duplicates", config=config, rows=n,
                            columns=spec.get("only", everything)))
    return out


def case_subset(case: dict) -> list[str]:
    """The key columns a case's filter looks at."""
    config = case["config"]
    if config.get("columns"):
        return list(config["columns"])
    if config.get("column_prefix"):
        return [c for c in case["columns"] if c.startswith(config["column_prefix"])]
    return list(case["columns"])


def expected_rows(case: dict, table: dict) -> np.ndarray:
    """The positions of ``table``'s rows that the case's filter returns, in its order — this file's statement."""
    keys = table_keys(table, case_subset(case))
    return stable_order(keys) if case["filter"] == "sort_by" else first_occurrences(keys)


# ---- the golden file ---------------------------------------------------------------------------------------------------------------------------
def encode(column) -> dict:
    """A column as JSON: float64 / float32 as integer bit patterns, datetimes as int64 nanoseconds, strings with ``null`` for missing."""
    a = np.asarray(column)
    if a.dtype == np.float64:
        return {"dtype": "float64", "bits": a.view(np.uint64).tolist()}
    if a.dtype == np.float32:
        return {"dtype": "float32", "bits": a.view(np.uint32).tolist()}
    if a.dtype.kind == "M":
        return {"dtype": "datetime64[ns]", "ns": a.astype("datetime64[ns]").view(np.int64).tolist()}
    if a.dtype.kind == "b":
        return {"dtype": "bool", "values": a.astype(np.int64).tolist()}
    if a.dtype.kind in "iu":
        return {"dtype": str(a.dtype), "values": a.tolist()}
    return {"dtype": "object", "values": [None if (v is None or v != v) else str(v) for v in a.tolist()]}


def decode(record: dict) -> np.ndarray:
    dtype = record["dtype"]
    if dtype == "float64":
        return np.array(record["bits"], dtype=np.uint64).view(np.float64)
    if dtype == "float32":
        return np.array(record["bits"], dtype=np.uint32).view(np.float32)
    if dtype == "datetime64[ns]":
        return np.array(record["ns"], dtype=np.int64).view("datetime64[ns]")
    if dtype == "bool":
        return np.array(record["values"], dtype=np.int64) != 0
    if dtype == "object":
        out = np.empty(len(record["values"]), dtype=object)
        out[:] = record["values"]
        return out
    return np.array(record["values"], dtype=dtype)


def digest(columns: dict) -> str:
    """sha256 over the names, dtypes and BYTES of the columns in order (an object column by its ``repr``): what the golden file keeps
    of a frame that came out, beside its index labels."""
    h = hashlib.sha256()
    for name, col in columns.items():
        a = np.asarray(col)
        h.update(f"{name}:{a.dtype}:".encode())
        h.update(repr(a.tolist()).encode() if a.dtype.kind == "O" else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def load_golden() -> dict:
    """``{"tables": {name: {"index": labels, "columns": {name: array}}}, "cases": [...]}`` with every column decoded; a case holds
    ``id``, ``filter``, ``config``, ``table`` (a name), ``columns`` (those of the table the filter saw), ``index`` (the labels that came
    out) and ``expected`` (the columns that came out).  The file keeps the index labels and a ``digest`` of the columns of every frame;
    the labels are unique, so ``expected`` is the table's rows at those labels — and must have the recorded digest, bit for bit."""
    with open(GOLDEN) as f:
        raw = json.load(f)
    tables = {name: {"index": np.array(t["index"], dtype=np.int64), "columns": {c: decode(v) for c, v in t["columns"].items()}}
              for name, t in raw["tables"].items()}
    cases = []
    for case in raw["cases"]:
        table = tables[case["table"]]
        position = {label: p for p, label in enumerate(table["index"].tolist())}
        rows = np.array([position[label] for label in case["index"]], dtype=np.int64)
        expected = {c: table["columns"][c][rows] for c in case["expected_columns"]}
        assert digest(expected) == case["digest"], case["id"]
        cases.append({**case, "index": np.array(case["index"], dtype=np.int64), "expected": expected})
    return {"tables": tables, "cases": cases}


def same_bits(a, b) -> bool:
    """Equal dtype, shape and BITS (a NaN's payload, the sign of a zero); object columns by value with ``None`` equal to ``None``."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "O":
        return a.tolist() == b.tolist()
    return a.tobytes() == b.tobytes()
