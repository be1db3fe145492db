"""The row programs of the tabular QC filters, restated without the package: a plain numpy interpreter of the operation table of
``atx_obs_column_ops``' second family (include/atx.h: slots, ``src``, ``y`` = the result of the slot before, launch boundaries) and the
nine filters' statements in plain numpy, compared on bit patterns.  Also the seeded tables and configurations that
``tools/record_obs_qc_golden.py`` ran through the reference's own ``forward`` (tests/golden/obs_qc.json), and random configurations.

A helper, not a test file.  Used by tests/test_obs_qc_host.py, tests/test_gpu_obs_qc.py and tests/test_obs_qc_checks_catch_defects.py.
"""

from __future__ import annotations

import json
import os

import numpy as np

from rowset_restatement import decode, digest, encode, same_bits  # noqa: F401  (the golden files share one encoding)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obs_qc.json")
MAX_OPS = 16
CODES = {"scalar": 16, "copy": 17, "is_nan": 18, "not": 19, "cmp_gt": 20, "cmp_lt": 21, "cmp_eq": 22, "cmp_ne": 23, "cmp_ge": 24,
         "cmp_le": 25, "abs_gt": 26, "and": 27, "or": 28, "nan_where": 29, "clip_low": 30, "clip_high": 31, "fill_nan": 32}
NAMES = {code: name for name, code in CODES.items()}
BINARY = {name for name, code in CODES.items() if code >= 20}
QUIET_NAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
DBL_MAX = np.finfo(np.float64).max
DAY_NS = 86400 * 10**9
NAT = np.iinfo(np.int64).min
DEFECTS = ("ge_as_gt", "nan_where_inverted", "y_from_two_back")  # what the interpreter can be told to get wrong


# ---- the interpreter ---------------------------------------------------------------------------------------------------------------------
def _flag(c: np.ndarray) -> np.ndarray:
    return np.where(c, 1.0, 0.0)


def apply(name: str, x: np.ndarray, y: np.ndarray | None, defect: str | None = None) -> np.ndarray:
    """One operation of the table over whole rows.  ``np.where`` hands on the bits of the operand it picks."""
    with np.errstate(invalid="ignore"):
        if name in ("scalar", "copy"):
            return x.copy()
        if name == "is_nan":
            return _flag(x != x)
        if name == "not":
            return _flag(x == 0)
        if name == "cmp_gt" or (name == "cmp_ge" and defect == "ge_as_gt"):
            return _flag(x > y)
        if name == "cmp_lt":
            return _flag(x < y)
        if name == "cmp_eq":
            return _flag(x == y)
        if name == "cmp_ne":
            return _flag(x != y)
        if name == "cmp_ge":
            return _flag(x >= y)
        if name == "cmp_le":
            return _flag(x <= y)
        if name == "abs_gt":
            return _flag(np.abs(x) > y)
        if name == "and":
            return _flag((x != 0) & (y != 0))
        if name == "or":
            return _flag((x != 0) | (y != 0))
        if name == "nan_where":
            return np.where((y == 0) if defect == "nan_where_inverted" else (y != 0), QUIET_NAN, x)
        if name == "clip_low":
            return np.where(x < y, y, x)
        if name == "clip_high":
            return np.where(x > y, y, x)
        if name == "fill_nan":
            return np.where(x != x, y, x)
    raise ValueError(name)


def launch(ops, n: int, defect: str | None = None) -> None:
    """What one call of ``atx_obs_column_ops`` does, with numpy arrays for device rows: ``ops`` is a list of ``(code, src, column, out)``;
    ``column`` of a SCALAR is an array of which element 0 is read; ``out`` is written in place or is None.  Every input is read before
    any output is written only where the kernel does so too: slot by slot, in order."""
    assert 1 <= len(ops) <= MAX_OPS
    results: list[np.ndarray] = []
    for t, (code, src, column, out) in enumerate(ops):
        name = NAMES[int(code)]
        assert src < t and (name not in BINARY or t > 0) and (name != "scalar" or src < 0)
        if name == "scalar":
            x = np.full(n, np.asarray(column, dtype=np.float64).reshape(-1)[0])
        elif src < 0:
            x = np.array(column, dtype=np.float64, copy=True)
            assert x.shape == (n,)
        else:
            x = results[src]
        back = 2 if (defect == "y_from_two_back" and t >= 2) else 1
        y = results[t - back] if t > 0 else None
        results.append(apply(name, x, y, defect))
        if out is not None:
            out[:] = results[-1]


def run_program(program, table: dict, rows: dict | None = None, defect: str | None = None) -> dict:
    """``obs.row_program`` in numpy: a ``RowProgram`` (anything with ``scalars``, ``launches`` of ``slots`` with ``op``, ``src``, ``read``,
    ``scalar``, ``store``, and ``results``) over a table of numpy columns.  A stored row reaches later launches through memory."""
    scalars = np.asarray(program.scalars, dtype=np.float64)
    memory = {name: np.asarray(col, dtype=np.float64) for name, col in (rows or {}).items()}
    written: dict[str, np.ndarray] = {}

    def row(name):
        if name in written:
            return written[name]
        if name not in memory:
            memory[name] = np.asarray(table[name]).astype(np.float64)
        return memory[name]

    for one in program.launches:
        n = next(len(row(s.read)) for s in one.slots if s.read is not None)
        outs = [np.empty(n) if s.store is not None else None for s in one.slots]
        launch([(CODES[s.op], s.src, scalars[s.scalar:s.scalar + 1] if s.op == "scalar" else (row(s.read) if s.read is not None else None), o)
                for s, o in zip(one.slots, outs)], n, defect)
        written.update({s.store: o for s, o in zip(one.slots, outs) if o is not None})
    return {name: written[name] for name in program.results}


# ---- the nine statements, in plain numpy --------------------------------------------------------------------------------------------------
NUMPY_OPERATORS = {">": np.greater, "<": np.less, "==": np.equal, "!=": np.not_equal, ">=": np.greater_equal, "<=": np.less_equal,
                   "gt": np.greater, "lt": np.less, "eq": np.equal, "ne": np.not_equal, "ge": np.greater_equal, "le": np.less_equal}


def masked(column: np.ndarray, cond: np.ndarray) -> np.ndarray:
    """``Series.mask(cond)``: NaN where ``cond``; a float column keeps its dtype, an integer one becomes float64 only if a row is masked."""
    column = np.asarray(column)
    if column.dtype.kind != "f":
        if not cond.any():
            return column
        column = column.astype(np.float64)
    return np.where(cond, column.dtype.type(QUIET_NAN), column)


def _selection(table: dict, config: dict) -> list[str] | None:
    if config.get("columns"):
        return list(config["columns"])
    if config.get("column_prefix"):
        return [c for c in table if c.startswith(config["column_prefix"])]
    return None


def utc_days(date: np.ndarray) -> np.ndarray:
    ns = np.asarray(date).astype("datetime64[ns]").view(np.int64)
    return np.where(ns == NAT, np.nan, (ns // DAY_NS).astype(np.float64))


def epoch_day(value) -> int:
    s = str(value)
    return int((np.datetime64(f"{s[:4]}-{s[4:6]}-{s[6:8]}") - np.datetime64("1970-01-01")) // np.timedelta64(1, "D"))


def is_missing(column: np.ndarray) -> np.ndarray:
    column = np.asarray(column)
    if column.dtype.kind == "f":
        return np.isnan(column)
    if column.dtype.kind == "M":
        return np.isnat(column)
    if column.dtype.kind == "O":
        return np.array([v is None or v != v for v in column.tolist()], dtype=bool)
    return np.zeros(len(column), dtype=bool)


def statement(filter_name: str, config: dict, table: dict, round_scalars: bool = True, q_by_masked_td: bool = False):
    """``("columns", {name: column})`` — the columns the filter replaces — or ``("rows", positions)`` — the rows it keeps.  numpy compares
    a float32 column with a Python number in float32 by itself (``round_scalars=False`` widens the column first: a defect to catch)."""
    def col(name):
        c = np.asarray(table[name])
        return c if round_scalars or c.dtype.kind != "f" else c.astype(np.float64)

    def narrow(name, result):
        dtype = np.asarray(table[name]).dtype
        return result.astype(dtype) if dtype.kind == "f" and result.dtype != dtype else result

    with np.errstate(invalid="ignore", over="ignore"):
        if filter_name == "mask_tabular":
            return "columns", {c: narrow(c, masked(col(c), NUMPY_OPERATORS[spec.get("operator", "==")](col(c), spec["value"]))) for c, spec in config.items()}
        if filter_name == "mask_outside_range":
            out = {}
            for c, (low, high) in config.items():
                x = col(c)
                cond = (x < low if low is not None else np.zeros(len(x), bool)) | (x > high if high is not None else np.zeros(len(x), bool))
                out[c] = narrow(c, masked(x, cond))
            return "columns", out
        if filter_name == "mask_infs":
            return "columns", {c: masked(np.asarray(table[c]), np.isinf(np.asarray(table[c]).astype(np.float64))) for c in _selection(table, config)}
        if filter_name == "mask_dewpoint_temperature":
            t, td, q = config.get("temperature", "2t"), config.get("dewpoint_temperature", "2d"), config.get("specific_humidity", "2q")
            cond = np.asarray(table[t]) < np.asarray(table[td])
            out = {td: masked(table[td], cond)}
            if config.get("mask_specific_humidity", False):
                out[q] = masked(table[q], (np.asarray(table[t]) < out[td]) if q_by_masked_td else cond)
            return "columns", out
        if filter_name == "exclude_dates":
            day = utc_days(table["date"])
            out = {}
            for c, ranges in config.items():
                if len(ranges) == 2 and all(isinstance(r, (int, str)) for r in ranges):
                    ranges = [ranges]
                cond = np.zeros(len(day), dtype=bool)
                for start, end in ranges:
                    cond |= (day >= epoch_day(start)) & (day < epoch_day(end) + 1)
                out[c] = masked(table[c], cond)
            return "columns", out
        if filter_name == "remove_extreme_values":
            names = list(dict.fromkeys(_selection(table, config) + ["latitude", "longitude"]))
            beyond = {c: np.abs(col(c)) > config.get("threshold", 1e10) for c in names}
            if config.get("method", "drop") == "mask":
                return "columns", {c: narrow(c, masked(col(c), beyond[c])) for c in names}
            return "rows", np.nonzero(~np.logical_or.reduce([beyond[c] for c in names]))[0]
        if filter_name == "clip_tabular":
            out = {}
            for c, (low, high) in config.items():
                x = np.asarray(table[c])
                low, high = (None if v is None or v != v else v for v in (low, high))
                if low is not None and high is not None and low > high:
                    low, high = high, low
                y = x if x.dtype.kind == "f" else x.astype(np.float64)
                bound = (lambda v: y.dtype.type(v)) if round_scalars or x.dtype.kind != "f" else np.float64
                if not round_scalars and x.dtype.kind == "f":
                    y = y.astype(np.float64)
                if low is not None:
                    y = np.where(y < bound(low), bound(low), y)
                if high is not None:
                    y = np.where(y > bound(high), bound(high), y)
                if x.dtype.kind != "f":
                    y = y.astype(x.dtype) if (y == np.floor(y)).all() else y  # pandas: an integer column holds whole numbers
                out[c] = narrow(c, y) if (low is not None or high is not None) else x
            return "columns", {c: v for c, v in out.items()}
        if filter_name == "impute_nans_tabular":
            value = config["value"]
            out = {}
            for c in table:
                x = np.asarray(table[c])
                if x.dtype.kind == "f" and (not isinstance(value, dict) or c in value):
                    v = value[c] if isinstance(value, dict) else value
                    out[c] = np.where(np.isnan(x), x.dtype.type(v), x)
            return "columns", out
        if filter_name == "drop_nans_tabular":
            subset = _selection(table, config) or list(table)
            missing = [is_missing(table[c]) for c in subset]
            gone = np.logical_or.reduce(missing) if config.get("how", "any") == "any" else np.logical_and.reduce(missing)
            return "rows", np.nonzero(~gone)[0]
    raise ValueError(filter_name)


# ---- seeded tables and configurations ------------------------------------------------------------------------------------------------------
SEEDED_ROWS = (48, 300)
THRESHOLDS = (0.1, 2.5, -3.0, 1e10, 273.15)  # 0.1 and 273.15 are no float32 numbers: the float32 compare differs from the float64 one


def _around(t: float) -> list[float]:
    f = np.float32(t)
    return [t, float(f), float(np.nextafter(f, np.float32(np.inf))), float(np.nextafter(f, np.float32(-np.inf))),
            float(np.nextafter(t, np.inf)), float(np.nextafter(t, -np.inf)), -t]


def value_pool() -> np.ndarray:
    pool = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, DBL_MAX, -DBL_MAX, 3.0e38, 5e-324]
    for t in THRESHOLDS:
        pool += _around(t)
    return np.array(pool, dtype=np.float64)


def seeded_table(n: int) -> dict:
    """``n`` rows.  ``a``, ``obsvalue_x`` float64 and ``b``, ``obsvalue_y`` float32 run through ``value_pool`` first (every special, every
    threshold and one float32 ulp either side of it) and are random beyond; ``i`` int64 has rows that every configuration masks, ``j``
    int64 none; ``2t`` / ``2d`` / ``2q`` float64 / float32 / int64; ``latitude`` / ``longitude`` float64 with a few beyond 1e10; ``date``
    datetimes over twelve days with NaT; ``s`` strings with None; ``label``: the DataFrame's index labels, not 0 .. n - 1."""
    rng = np.random.default_rng(9100 + n)
    pool = value_pool()

    def values(scale):
        v = rng.choice(pool, n)
        v = np.where(rng.random(n) < 0.5, v, rng.standard_normal(n) * scale)
        v[:len(pool)] = pool[:n]
        return v[rng.permutation(n)]

    with np.errstate(over="ignore"):
        table = {"a": values(3.0), "b": values(3.0).astype(np.float32), "obsvalue_x": values(1e10), "obsvalue_y": values(280.0).astype(np.float32)}
    table["i"] = rng.integers(-6, 7, n).astype(np.int64)
    table["j"] = rng.integers(0, 2, n).astype(np.int64)
    table["2t"] = 273.15 + rng.integers(-3, 4, n).astype(np.float64)
    table["2t"][rng.random(n) < 0.1] = np.nan
    table["2d"] = (273.15 + rng.integers(-3, 4, n)).astype(np.float32)
    table["2d"][rng.random(n) < 0.1] = np.nan
    table["2q"] = rng.integers(1, 20, n).astype(np.int64)
    table["latitude"] = rng.uniform(-90, 90, n)
    table["longitude"] = rng.uniform(-180, 180, n)
    table["latitude"][rng.random(n) < 0.05] = 2e10
    table["longitude"][rng.random(n) < 0.05] = -np.inf
    table["longitude"][rng.random(n) < 0.05] = np.nan
    ns = np.datetime64("2024-12-28T00:00", "ns").view(np.int64) + rng.integers(0, 12 * 24, n) * (3600 * 10**9)
    ns[rng.random(n) < 0.1] = NAT
    ns[:3] = [np.datetime64("2025-01-01T00:00", "ns").view(np.int64), np.datetime64("2025-01-02T23:59:59.999999999", "ns").view(np.int64),
              np.datetime64("2025-01-03T00:00", "ns").view(np.int64)]
    table["date"] = ns.view("datetime64[ns]")
    s = np.empty(n, dtype=object)
    s[:] = [None if rng.random() < 0.15 else f"st{int(k)}" for k in rng.integers(0, 9, n)]
    table["s"] = s
    table["label"] = (1000 + 7 * rng.permutation(n)).astype(np.int64)
    return table


SEEDED_CONFIGS = (
    ("mask_tabular", {"a": {"value": 0.1}, "b": {"value": 0.1, "operator": ">"}, "i": {"value": 2, "operator": ">="}, "j": {"value": 5, "operator": "gt"}}),
    ("mask_tabular", {"a": {"value": 2.5, "operator": "le"}, "b": {"value": 0.1, "operator": "=="}, "obsvalue_y": {"value": 273.15, "operator": "<"},
                      "i": {"value": -3.0, "operator": "!="}}),
    ("mask_tabular", {"b": {"value": 0.1, "operator": "ne"}, "obsvalue_y": {"value": 273.15, "operator": "ge"}, "a": {"value": -3.0, "operator": "lt"},
                      "obsvalue_x": {"value": 1e10, "operator": "eq"}, "i": {"value": 100, "operator": "<="}}),
    ("mask_outside_range", {"a": [-3.0, 2.5], "b": [-3.0, 0.1], "obsvalue_y": [273.15, None], "i": [-3, 2.5], "j": [0, 1]}),
    ("mask_infs", {"columns": ["a", "b", "i"]}),
    ("mask_infs", {"column_prefix": "obsvalue_"}),
    ("mask_dewpoint_temperature", {}),
    ("mask_dewpoint_temperature", {"mask_specific_humidity": True}),
    ("mask_dewpoint_temperature", {"temperature": "b", "dewpoint_temperature": "a", "specific_humidity": "obsvalue_y", "mask_specific_humidity": True}),
    ("exclude_dates", {"a": [[20250101, 20250102], ["20250105", "20250105"]], "i": [20241230, 20241230], "j": [[19990101, 19990102]],
                       "b": [[20241228, 20241229], [20250103, 20250104], [20250107, 20250107]]}),
    ("remove_extreme_values", {"columns": ["obsvalue_x", "obsvalue_y"], "method": "mask"}),
    ("remove_extreme_values", {"column_prefix": "obsvalue_", "method": "drop"}),
    ("remove_extreme_values", {"columns": ["obsvalue_y", "b", "i"], "threshold": 273.15, "method": "drop"}),
    ("remove_extreme_values", {"columns": ["b"], "threshold": 0.1, "method": "mask"}),
    ("clip_tabular", {"a": [-3.0, 2.5], "b": [0.1, None], "obsvalue_y": [None, 273.15], "i": [-3, 2], "j": [0.5, None], "2q": [0.0, 10.0]}),
    ("clip_tabular", {"a": [2.5, -3.0], "b": [0.1, 2.5], "i": [None, 2.5], "obsvalue_x": [float("nan"), 1e10]}),
    ("impute_nans_tabular", {"value": 0.1}),
    ("impute_nans_tabular", {"value": {"a": -1.0, "b": 273.15, "i": 7}, "columns": ["a"]}),
    ("drop_nans_tabular", {}),
    ("drop_nans_tabular", {"how": "all", "columns": ["date", "s"]}),
    ("drop_nans_tabular", {"how": "all", "columns": ["a", "2d", "i"]}),
    ("drop_nans_tabular", {"how": "all", "columns": ["b"]}),
    ("drop_nans_tabular", {"how": "any", "column_prefix": "obsvalue_"}),
    ("drop_nans_tabular", {"how": "any", "columns": ["date", "s", "i"]}),
)
# impute_nans_tabular with a scalar fills the date and the string column through pandas: a DataFrame alone can hold the result
FRAME_ONLY = {"impute_nans_tabular"}


def seeded_cases() -> list[dict]:
    return [dict(id=f"seeded_{n}_{k:02d}_{name}", filter=name, config=config, table=f"seeded_{n}")
            for n in SEEDED_ROWS for k, (name, config) in enumerate(SEEDED_CONFIGS)]


def random_config(rng: np.random.Generator) -> tuple[str, dict]:
    """One filter and a configuration over the seeded table's numeric columns, thresholds from ``THRESHOLDS`` and around them."""
    floats, ints = ["a", "b", "obsvalue_x", "obsvalue_y"], ["i", "j", "2q"]
    numeric = floats + ints

    def some(names, low=1, high=None):
        return [str(c) for c in rng.choice(names, size=int(rng.integers(low, (high or len(names)) + 1)), replace=False)]

    def number():
        v = float(rng.choice(_around(float(rng.choice(THRESHOLDS)))))
        return int(rng.integers(-4, 5)) if rng.random() < 0.25 else v

    def bounds():
        return [None if rng.random() < 0.25 else number(), None if rng.random() < 0.25 else number()]

    name = str(rng.choice(["mask_tabular", "mask_outside_range", "mask_infs", "mask_dewpoint_temperature", "exclude_dates", "remove_extreme_values",
                           "clip_tabular", "impute_nans_tabular", "drop_nans_tabular"]))
    if name == "mask_tabular":
        return name, {c: {"value": number(), "operator": str(rng.choice(list(NUMPY_OPERATORS)))} for c in some(numeric)}
    if name == "mask_outside_range":
        return name, {c: bounds() for c in some(numeric)}
    if name == "mask_infs":
        return name, ({"columns": some(numeric)} if rng.random() < 0.7 else {"column_prefix": "obsvalue_"})
    if name == "mask_dewpoint_temperature":
        t, td, q = some(numeric, 3, 3)
        return name, {"temperature": t, "dewpoint_temperature": td, "specific_humidity": q, "mask_specific_humidity": bool(rng.random() < 0.6)}
    if name == "exclude_dates":
        def day():
            return int(str(np.datetime64("2024-12-26") + int(rng.integers(0, 16))).replace("-", ""))
        return name, {c: [sorted([day(), day()]) for _ in range(int(rng.integers(1, 7)))] for c in some(numeric, 1, 4)}
    if name == "remove_extreme_values":
        return name, {"columns": some(numeric, 1, 7), "threshold": abs(number()), "method": str(rng.choice(["mask", "drop"]))}
    if name == "clip_tabular":
        return name, {c: bounds() for c in some(numeric)}
    if name == "impute_nans_tabular":
        return name, {"value": ({c: number() for c in some(floats)} if rng.random() < 0.5 else number())}
    return name, {"how": str(rng.choice(["any", "all"])), "columns": some(numeric + ["date", "s", "2t", "2d"], 1, 11)}


# ---- the golden file -----------------------------------------------------------------------------------------------------------------------
def pack_rows(flags: np.ndarray) -> str:
    """A set of rows as the hex digits of its bit mask, row 0 first."""
    return np.packbits(np.asarray(flags, dtype=bool)).tobytes().hex()


def unpack_rows(digits: str, n: int) -> np.ndarray:
    return np.unpackbits(np.frombuffer(bytes.fromhex(digits), dtype=np.uint8))[:n].astype(bool)


def _listed(record: dict) -> list:
    return record[next(key for key in record if key != "dtype")]


def _start(base: np.ndarray, dtype: str) -> np.ndarray:
    return base if dtype == "object" or str(base.dtype) == dtype else base.astype(dtype)  # int64 -> float64: exact below 2**53


def pack_changed(base: np.ndarray, after: np.ndarray) -> dict:
    """A column that came out as the golden file keeps it: its dtype and, per distinct new value, the rows that hold it (``patches``);
    every other row holds the table's value, cast to that dtype.  A column that this cannot restate to the bit (a datetime column that
    came back as objects) is kept whole (``full``)."""
    whole = encode(after)
    record = {"full": whole}
    if whole["dtype"] != "object" or base.dtype.kind == "O":
        new, old = _listed(whole), _listed(encode(_start(base, whole["dtype"])))
        values = []
        for a, b in zip(new, old):
            if a != b and a not in values:
                values.append(a)
        record = {"dtype": whole["dtype"], "patches": [[pack_rows([a == v and a != b for a, b in zip(new, old)]), v] for v in values]}
    assert same_bits(unpack_changed(base, record), decode(whole))
    return record


def unpack_changed(base: np.ndarray, record: dict) -> np.ndarray:
    if "full" in record:
        return decode(record["full"])
    whole = encode(_start(base, record["dtype"]))
    listed = _listed(whole)
    for digits, value in record["patches"]:
        for k in np.flatnonzero(unpack_rows(digits, len(listed))):
            listed[k] = value
    return decode(whole)


def load_golden() -> dict:
    """``{"tables": {name: {"index": labels, "columns": {name: array}}}, "cases": [...]}``; a case holds ``id``, ``filter``, ``config``,
    ``table``, ``index`` (the labels that came out), ``changed`` (the columns that differ from the table's, decoded), ``dtypes`` (of every
    column that came out) and ``digest`` (of the whole frame that came out).  The file keeps a seeded table as its row count and digest,
    the labels as the set of rows that left (``dropped``), a changed column as ``pack_changed`` writes it and the dtypes that changed."""
    with open(GOLDEN) as f:
        raw = json.load(f)
    tables = {}
    for name, t in raw["tables"].items():
        if "seeded" in t:
            columns = seeded_table(t["seeded"])
            assert frame_digest(columns) == t["digest"], name
            tables[name] = {"index": columns.pop("label"), "columns": columns}
        else:
            tables[name] = {"index": np.array(t["index"], dtype=np.int64), "columns": {c: decode(v) for c, v in t["columns"].items()}}
    cases = []
    for case in raw["cases"]:
        table = tables[case["table"]]
        n = len(table["index"])
        rows = np.flatnonzero(~unpack_rows(case["dropped"], n)) if "dropped" in case else np.arange(n)
        case = {key: value for key, value in case.items() if key != "dropped"}
        case["index"] = table["index"][rows]
        case["changed"] = {c: unpack_changed(table["columns"][c][rows], record) for c, record in case["changed"].items()}
        case["dtypes"] = {c: case["dtypes"].get(c, str(v.dtype)) for c, v in table["columns"].items()}
        cases.append(case)
    return {"tables": tables, "cases": cases}


def frame_digest(columns: dict) -> str:
    """``digest`` with every object column as the golden file keeps it (strings, None): a filled datetime column holds Timestamps."""
    return digest({c: (decode(encode(v)) if np.asarray(v).dtype.kind == "O" else v) for c, v in columns.items()})


def expected_frame(golden: dict, case: dict) -> dict:
    """The columns of the frame the reference returned: the table's rows at the surviving labels, with the changed columns put in."""
    table = golden["tables"][case["table"]]
    at = {int(label): k for k, label in enumerate(table["index"])}
    rows = np.array([at[int(label)] for label in case["index"]], dtype=np.int64)
    out = {c: (case["changed"][c] if c in case["changed"] else v[rows]) for c, v in table["columns"].items()}
    assert {c: str(v.dtype) for c, v in out.items()} == case["dtypes"] and frame_digest(out) == case["digest"], case["id"]
    return out


def same_column(got, want: np.ndarray) -> bool:
    """A column that came out against the recorded one: dtype and bits; an object column by its encoded values (a filled datetime column
    holds Timestamps and numbers)."""
    if isinstance(got, np.ndarray) and got.dtype.kind == "M" and want.dtype.kind == "M":
        return same_bits(got.astype("datetime64[ns]"), want)
    if want.dtype.kind == "O":
        return encode(np.asarray(got, dtype=object))["values"] == want.tolist()
    return same_bits(got, want)


def input_table(golden: dict, case: dict, kind: str, device=None):
    """The case's table as a DataFrame (``"frame"``, with its index labels), a dict of numpy arrays (``"host"``) or a dict of device tensors
    (``"device"``: numeric columns as tensors, datetimes as int64 nanoseconds, strings left on the host)."""
    table = golden["tables"][case["table"]]
    if kind == "frame":
        import pandas as pd

        return pd.DataFrame(dict(table["columns"]), index=table["index"])
    if kind == "host":
        return {c: v.copy() for c, v in table["columns"].items()}
    import torch

    return {c: (v.copy() if v.dtype.kind == "O" else torch.from_numpy(v.view(np.int64).copy() if v.dtype.kind == "M" else v.copy()).to(device))
            for c, v in table["columns"].items()}


def check_case(got, golden: dict, case: dict, kind: str) -> None:
    """What a filter returned for ``input_table(golden, case, kind)`` against what the reference returned: the columns in order, every
    dtype, every bit, and for a DataFrame the index labels.  Device tensors are compared as what they hold (datetimes: nanoseconds)."""
    want = expected_frame(golden, case)
    assert list(got.keys() if kind != "frame" else got.columns) == list(want), case["id"]
    if kind == "frame":
        assert [int(i) for i in got.index] == [int(i) for i in case["index"]], case["id"]
    for name, column in want.items():
        g = got[name]
        if kind == "frame":
            g = g.to_numpy()
        elif kind == "device" and not isinstance(g, np.ndarray):
            g = g.cpu().numpy()
            column = column.view(np.int64) if column.dtype.kind == "M" else column
        assert same_column(g, column), (case["id"], kind, name, g[:8], column[:8])


def install_double(monkeypatch) -> None:
    """``native.obs_column_ops`` answered by ``launch`` on host tensors, and this process's device the host: the Python layers of the
    filters run where there is no GPU.  ``Table.take`` of a resident mapping still needs the device."""
    import torch

    from anemoi_transform_amd import native, stack

    def obs_column_ops(ops, n):
        launch([(code, src, None if column is None else column.numpy(), None if out is None else out.numpy()) for code, src, column, out in ops], n)

    monkeypatch.setattr(native, "obs_column_ops", obs_column_ops)
    monkeypatch.setattr(stack, "device", lambda: torch.device("cpu"))
