"""``sort_by``, ``drop_duplicates`` and ``drop`` without a GPU: the registry names, the constructor and missing-column errors as the
reference's tests state them, the header and binding of the three entry points and their argument checks, the numpy restatement
(tests/rowset_restatement.py) against pandas itself and against the recorded frames (tests/golden/rowset.json), and the conditions
that keep the seeded tables from going trivial.
"""

from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import rowset_restatement as R
from anemoi_transform_amd import native
from anemoi_transform_amd.filters import create_filter_by_name, filter_registry
from anemoi_transform_amd.filters.tabular import Drop, DropDuplicates, SortBy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = R.load_golden()
SEEDED = R.seeded_cases()


def _table(case: dict) -> dict:
    table = R.seeded_table(case["rows"])
    return {c: table[c] for c in case["columns"]}


def _frame(case: dict):
    import pandas as pd

    return pd.DataFrame(_table(case), index=R.seeded_table(case["rows"])["label"])


# ---- registration, construction, lookup -----------------------------------------------------------------------------------------------------
def test_registered_names_and_classes():
    assert {"sort_by", "drop_duplicates", "drop"} <= set(filter_registry.registered)
    assert isinstance(create_filter_by_name("sort_by", columns=["a", "b"]), SortBy)
    assert isinstance(create_filter_by_name("drop_duplicates"), DropDuplicates)
    assert isinstance(create_filter_by_name("drop_duplicates", column_prefix="obsvalue_"), DropDuplicates)
    assert isinstance(create_filter_by_name("drop", columns=["a"]), Drop)
    assert repr(create_filter_by_name("sort_by", columns=["a", "b"])) == "SortBy(['a', 'b'])"


def test_constructor_errors_are_the_reference_ones():
    with pytest.raises(ValueError, match="No columns to drop were specified."):  # R: tests/tabular_filters/test_drop.py:37-42
        create_filter_by_name("drop", columns=[])
    with pytest.raises(ValueError, match="not both"):  # R: filters/tabular/drop_duplicates.py:43-44
        create_filter_by_name("drop_duplicates", columns=["x"], column_prefix="obs")


@pytest.mark.parametrize("kind", ["frame", "mapping"])
def test_missing_columns_raise_value_error_before_any_launch(kind):
    """R: test_sort_by.py:52-67, test_drop_duplicates.py:41-55, test_drop.py:45-58 — the ``ValueError`` of ``_require``."""
    pd = pytest.importorskip("pandas")
    columns = {"col2": np.array([4, 5, 3, 2, 1]), "col3": np.array([0, 1, 2, 3, 4])}
    table = pd.DataFrame(columns) if kind == "frame" else columns
    for name, config in (("sort_by", {"columns": ["col1"]}), ("drop_duplicates", {"columns": ["col1"]}), ("drop", {"columns": ["col1"]})):
        with pytest.raises(ValueError, match="DataFrame is missing columns: {'col1'}"):
            create_filter_by_name(name, **config)(table)
    with pytest.raises(ValueError, match="No columns starting with 'obsvalue_' found"):
        create_filter_by_name("drop_duplicates", column_prefix="obsvalue_")(table)


def test_drop_is_host_bookkeeping_and_copies_nothing():
    pd = pytest.importorskip("pandas")
    case = next(c for c in GOLDEN["cases"] if c["id"] == "reference_test_drop")
    table = GOLDEN["tables"][case["table"]]["columns"]
    f = create_filter_by_name("drop", **case["config"])
    got = f(pd.DataFrame(table))
    assert isinstance(got, pd.DataFrame) and tuple(got.columns) == ("x",) and got["x"].equals(pd.DataFrame(table)["x"])  # R: test_drop.py:17-34
    assert list(case["expected"]) == ["x"] and R.same_bits(got["x"].to_numpy(), case["expected"]["x"])
    out = f(table)
    assert out is not table and list(out) == ["x"] and out["x"] is table["x"] and list(table) == ["x", "drop_me"]


def test_an_empty_table_comes_back_empty_with_its_columns():
    pd = pytest.importorskip("pandas")
    empty = {"a": np.zeros(0), "b": np.zeros(0, dtype=np.int64)}
    for name, config in (("sort_by", {"columns": ["a"]}), ("drop_duplicates", {}), ("drop_duplicates", {"columns": ["b"]})):
        out = create_filter_by_name(name, **config)(empty)
        assert out is not empty and list(out) == ["a", "b"] and all(len(v) == 0 for v in out.values())
        frame = create_filter_by_name(name, **config)(pd.DataFrame(empty))
        assert list(frame.columns) == ["a", "b"] and len(frame) == 0


def test_sort_by_says_its_deviation_once(caplog):
    import logging

    from anemoi_transform_amd.core import reset_notes

    reset_notes()
    with caplog.at_level(logging.DEBUG, logger="anemoi_transform_amd"):
        create_filter_by_name("sort_by", columns=["a"])
        create_filter_by_name("sort_by", columns=["b"])
    said = [r for r in caplog.records if "returns the table unsorted" in r.getMessage()]
    assert [r.levelno for r in said] == [logging.INFO, logging.DEBUG]


def test_keys_that_cannot_be_ordered_raise_value_error_on_the_host():
    import torch

    from anemoi_transform_amd import obs

    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="uint64"):
        obs.order_keys(np.array([1, 2], dtype=np.uint64), cpu)
    with pytest.raises(ValueError, match="cannot be ordered"):
        obs.order_keys(np.array(["a", 1, None], dtype=object), cpu)
    with pytest.raises(ValueError, match="int64 nanoseconds"):
        obs.order_keys(torch.zeros(3, dtype=torch.int32), cpu, datetime=True)
    with pytest.raises(ValueError, match="at least one key column"):
        obs.sort_order([], cpu)
    # strings and categoricals are ranked on the host, missing last
    assert obs._host_ranks(np.array(["b", None, "a", "b"], dtype=object)).tolist() == [1, 2, 0, 1]
    pd = pytest.importorskip("pandas")
    cat = pd.Series(pd.Categorical(["lo", "hi", None, "lo"], categories=["lo", "hi"]))  # pandas sorts by the categories' order
    assert obs._host_ranks(cat).tolist() == [0, 1, 2, 0]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_cite_the_reference():
    header = open(os.path.join(ROOT, "include", "atx.h")).read()
    for name in ("atx_obs_order_key", "atx_obs_mark_first", "atx_obs_take_rows"):
        assert f"ATX_API int {name}(" in header and name in native.SIGNATURES
    assert "filters/tabular/sort_by.py" in header and "filters/tabular/drop_duplicates.py" in header
    assert f"#define ATX_MAX_ROWSET_COLUMNS {native.MAX_ROWSET_COLUMNS}" in header and "#define ATX_VERSION 420" in header
    for name, code in R.CODES.items():  # the codes of the header are the codes of the binding and of the restatement
        tag = {"float64": "F64", "float32": "F32", "datetime": "DATETIME", "bool": "BOOL"}.get(name, name.upper().replace("INT", "I").replace("UI", "U"))
        assert f"ATX_KEY_{tag} = {code}" in header and getattr(native, f"KEY_{tag}") == code
    assert len(native.SIGNATURES) == 57


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = native.load()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    EINVAL, OK = native.EINVAL, native.OK

    # atx_obs_order_key(column, n, dtype, key, stream)
    assert lib.atx_obs_order_key(one, -1, 0, one, None) == EINVAL
    assert lib.atx_obs_order_key(one, 8, 9, one, None) == EINVAL and b"key dtype 9" in lib.atx_last_error()
    assert lib.atx_obs_order_key(one, 8, -1, one, None) == EINVAL
    assert lib.atx_obs_order_key(None, 8, 0, one, None) == EINVAL and b"null pointer" in lib.atx_last_error()
    assert lib.atx_obs_order_key(one, 8, 0, None, None) == EINVAL
    assert lib.atx_obs_order_key(None, 0, 8, None, None) == OK  # no rows: validated, nothing launched

    # atx_obs_mark_first(n_keys, keys, order, n, accumulate, keep, stream)
    def mark(keys, order=one, n=8, accumulate=0, keep=one, n_keys=None):
        k = len(keys)
        return lib.atx_obs_mark_first(k if n_keys is None else n_keys, (ctypes.c_void_p * max(k, 1))(*keys), order, n, accumulate, keep, None)

    assert mark([one], n_keys=0) == EINVAL and b"1 .. 16 key columns" in lib.atx_last_error()
    assert mark([one] * 17) == EINVAL
    assert mark([one], n=-1) == EINVAL
    assert mark([one], accumulate=2) == EINVAL and b"accumulate 2" in lib.atx_last_error()
    assert mark([one, None]) == EINVAL and b"key column 1 is null" in lib.atx_last_error()
    assert mark([one], order=None) == EINVAL and mark([one], keep=None) == EINVAL
    assert lib.atx_obs_mark_first(1, None, one, 8, 0, one, None) == EINVAL and b"null key table" in lib.atx_last_error()
    assert mark([None] * 16, order=None, n=0, accumulate=1, keep=None) == OK

    # atx_obs_take_rows(n_cols, in, out, width, rows, n_out, n_in, n_bad, stream)
    def take(ins, outs, widths, rows=one, n_out=8, n_in=8, n_bad=one, n_cols=None):
        k = len(ins)
        return lib.atx_obs_take_rows(k if n_cols is None else n_cols, (ctypes.c_void_p * max(k, 1))(*ins), (ctypes.c_void_p * max(k, 1))(*outs),
                                     (ctypes.c_int32 * max(k, 1))(*widths), rows, n_out, n_in, n_bad, None)

    assert take([one], [one], [8], n_cols=0) == EINVAL and b"1 .. 16 columns" in lib.atx_last_error()
    assert take([one] * 17, [one] * 17, [8] * 17) == EINVAL
    for width in (0, 3, 5, 16, -1):
        assert take([one], [one], [width]) == EINVAL and b"1, 2, 4 or 8" in lib.atx_last_error()
    assert take([one], [one], [8], n_out=-1) == EINVAL and take([one], [one], [8], n_in=-1) == EINVAL
    assert take([one, None], [one, one], [8, 1]) == EINVAL and b"input column 1 is null" in lib.atx_last_error()
    assert take([one, one], [one, None], [8, 1]) == EINVAL and b"output column 1 is null" in lib.atx_last_error()
    assert take([one], [one], [8], rows=None) == EINVAL and b"null rows" in lib.atx_last_error()
    assert take([one], [one], [8], n_bad=None) == EINVAL and b"null n_bad" in lib.atx_last_error()
    assert lib.atx_obs_take_rows(1, None, None, None, one, 8, 8, one, None) == EINVAL and b"null column table" in lib.atx_last_error()
    assert take([one] * 16, [None] * 16, [1, 2, 4, 8] * 4, rows=None, n_out=0) == OK  # nothing to take: validated, nothing launched


# ---- the restatement against pandas and the recorded frames -----------------------------------------------------------------------------------
def test_key_map_on_the_specials():
    """The two defining properties on every pair of the float64 pool: the keys order as pandas sorts, and are equal where pandas sees
    duplicates."""
    key = R.order_key(R.F64_POOL).tolist()
    by_value = dict(zip(map(repr, R.F64_POOL.tolist()), key))
    assert key[0] == key[1] == 0  # 0.0 and -0.0
    assert key[2] == key[3] == key[4] == key[5] == R.I64_MAX  # NaNs of both signs, with a payload, signalling
    assert by_value["-inf"] < by_value["-1e+300"] < by_value["-1.5"] < by_value["-2.2250738585072014e-308"] < by_value["-5e-324"] < 0
    assert 0 < by_value["5e-324"] < by_value["1.0"] < by_value["1.0000000000000002"] < by_value["1.5"] < by_value["1e+300"] < by_value["inf"] < R.I64_MAX
    with np.errstate(invalid="ignore"):
        assert R.order_key(R.F32_POOL).tolist() == R.order_key(R.F32_POOL.astype(np.float64)).tolist()  # widened exactly
    assert R.order_key(R.I64_POOL).tolist() == R.I64_POOL.tolist() and 2**53 in R.I64_POOL and 2**53 + 1 in R.I64_POOL
    dates = R.order_key(R.DATE_POOL)
    assert dates[0] == R.I64_MAX and (dates[1:] == R.DATE_POOL.view(np.int64)[1:]).all() and (dates[1:3] < 0).all()
    assert R.order_key(np.array([True, False])).tolist() == [1, 0] and R.order_key(np.array([-128, 127], dtype=np.int8)).tolist() == [-128, 127]
    assert R.order_key(np.array([255], dtype=np.uint8)).tolist() == [255]
    for code in R.CODES:
        x = R.key_specials(code)
        keys = R.order_key(x, datetime=code == "datetime")
        assert keys.dtype == np.int64 and keys.size == x.size >= 200


def test_mark_first_restated_accumulates_and_never_clears():
    rng = np.random.default_rng(3)
    keys = [rng.integers(0, 3, 200) for _ in range(3)]
    order = R.stable_order(keys)
    whole = R.mark_first(keys, order)
    assert np.array_equal(np.nonzero(whole)[0], R.first_occurrences(keys))
    parts = R.mark_first(keys[2:], order, keep=R.mark_first(keys[:2], order))
    assert np.array_equal(parts, whole)
    assert np.array_equal(R.mark_first(keys, order, keep=np.ones(200, dtype=np.uint8)), np.ones(200, dtype=np.uint8))


@pytest.mark.parametrize("case", SEEDED, ids=[c["id"] for c in SEEDED])
def test_restatement_equals_pandas_on_the_seeded_tables(case):
    pytest.importorskip("pandas")
    frame = _frame(case)
    table = _table(case)
    rows = R.expected_rows(case, table)
    subset = R.case_subset(case)
    if case["filter"] == "sort_by":
        want = frame.sort_values(by=case["config"]["columns"], kind="stable")
    else:
        want = frame.drop_duplicates(subset=subset if (case["config"].get("columns") or case["config"].get("column_prefix")) else None)
    assert frame.index[rows].tolist() == want.index.tolist()

    # the conditions that keep the case from going trivial, on the pandas side
    sizes = frame.groupby(subset, dropna=False, sort=False)[subset[0]].transform("size")
    assert (sizes >= 2).sum() * 4 >= len(frame), f"{int((sizes >= 2).sum())} of {len(frame)} rows in groups of two or more"
    if case["filter"] == "sort_by":
        # a tie broken by table order alone: two adjacent sorted rows with equal key tuples
        dup = want.duplicated(subset=subset, keep="first").to_numpy()
        assert dup.any() and len(want) == len(frame)
        positions = {label: p for p, label in enumerate(frame.index)}
        sorted_positions = np.array([positions[label] for label in want.index])
        assert (np.diff(sorted_positions)[dup[1:]] > 0).all()  # within a tie, table order
    else:
        assert 1 < len(want) < len(frame)


def test_the_seeded_tables_hold_every_special_pandas_treats_its_own_way():
    pd = pytest.importorskip("pandas")
    for n in R.SEEDED_ROWS:
        table = R.seeded_table(n)
        assert 48 <= n <= 300 and all(len(v) == n for v in table.values())
        assert {table[c].dtype.kind for c in table} >= {"f", "i", "b", "M", "O"} and table["key_g"].dtype == np.float32
        frame = pd.DataFrame({c: v for c, v in table.items() if c != "label"}, index=table["label"])
        f = table["key_f"]
        # one group holds both zeros, one group NaNs of different sign and payload
        zeros = frame.index[(f == 0)]
        kept = frame.drop_duplicates(subset=["key_f"])
        assert (np.signbit(f[f == 0])).any() and (~np.signbit(f[f == 0])).any() and len(set(zeros) & set(kept.index)) == 1
        nan_bits = set(f[np.isnan(f)].view(np.uint64).tolist())
        assert len(nan_bits) >= 4 and any(b >> 63 for b in nan_bits) and any(not b >> 63 for b in nan_bits)
        assert len(set(frame.index[np.isnan(f)]) & set(kept.index)) == 1
        by_f = frame.sort_values(by=["key_f"], kind="stable")
        assert np.isnan(by_f["key_f"].to_numpy()[-int(np.isnan(f).sum()):]).all()  # missing last
        # NaT and dates before 1970 in one key column
        ns = table["date"].view(np.int64)
        assert (ns == R.I64_MIN).any() and ((ns < 0) & (ns != R.I64_MIN)).any()
        assert frame.sort_values(by=["date"], kind="stable")["date"].isna().to_numpy()[-int((ns == R.I64_MIN).sum()):].all()
        # int64 keys that float64 cannot tell apart, and the ends of the range
        k = table["key_k"]
        assert {2**53, 2**53 + 1, R.I64_MIN, R.I64_MAX} <= set(k.tolist())
        assert float(2**53) == float(2**53 + 1) and len(frame.drop_duplicates(subset=["key_k"])) == len(set(k.tolist()))
        assert None in table["name"].tolist() and "" in table["name"].tolist()


def test_restatement_equals_the_recorded_frames():
    """tests/golden/rowset.json: what the reference's own ``forward`` returned (tools/record_rowset_golden.py)."""
    ids = [c["id"] for c in GOLDEN["cases"]]
    assert ids[:5] == ["reference_test_sort_by", "reference_test_drop_duplicates", "reference_test_drop_duplicates_with_prefix",
                       "reference_test_drop_duplicates_no_config", "reference_test_drop"]
    assert ids[5:] == [c["id"] for c in SEEDED]
    for n in R.SEEDED_ROWS:  # the recorded tables are the builder's, bit for bit
        stored, built = GOLDEN["tables"][f"seeded_{n}"], R.seeded_table(n)
        assert stored["index"].tolist() == built["label"].tolist()
        assert all(R.same_bits(stored["columns"][c], built[c]) for c in stored["columns"]) and set(stored["columns"]) == set(built) - {"label"}
    for case in GOLDEN["cases"]:
        if case["filter"] == "drop":
            continue
        stored = GOLDEN["tables"][case["table"]]
        table = {c: stored["columns"][c] for c in case["columns"]}
        rows = R.expected_rows(case, table)
        assert stored["index"][rows].tolist() == case["index"].tolist(), case["id"]
        assert list(case["expected"]) == case["columns"]
        for name, column in case["expected"].items():
            assert R.same_bits(table[name][rows], column), (case["id"], name)
        if "literals" in case:  # R: tests/tabular_filters/test_sort_by.py:41-49
            assert all(table[c][rows].tolist() == v for c, v in case["literals"].items())
        if "dropped_index" in case:  # R: tests/tabular_filters/test_drop_duplicates.py:38, :77, :95
            assert case["index"].tolist() == [i for i in stored["index"].tolist() if i not in case["dropped_index"]]
