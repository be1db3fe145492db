"""The tabular QC filters without a device: the codes and argument checks of ``atx_obs_column_ops``' second family, the nine program
compilers against the plain numpy statements (tests/row_program_restatement.py) on the recorded cases and on random configurations, the
statements against the reference's own frames (tests/golden/obs_qc.json) and against pandas, the reference's constructor errors, and
which filter each dispatcher picks.  The kernel itself: tests/test_gpu_obs_qc.py.
"""

from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import row_program_restatement as R
from anemoi_transform_amd import native, obs
from anemoi_transform_amd.filters import create_filter_by_name, filter_registry
from anemoi_transform_amd.filters import tabular as T

GOLDEN = R.load_golden()
NINE = ("mask_tabular", "mask_outside_range", "mask_infs", "mask_dewpoint_temperature", "exclude_dates", "remove_extreme_values",
        "clip_tabular", "impute_nans_tabular", "drop_nans_tabular")


def compiled(name: str, config: dict, table: dict):
    """``(kind, program, rows)`` of a filter's configuration over ``table``: what its ``forward`` hands to ``obs.row_program``."""
    f = create_filter_by_name(name, **config)
    dtypes = {c: np.asarray(v).dtype for c, v in table.items()}
    rows = {}
    if name == "mask_tabular":
        program = obs.compile_mask_values(f.config, dtypes)
    elif name == "mask_outside_range":
        program = obs.compile_mask_outside_range({c: tuple(r) for c, r in f.config.items()}, dtypes)
    elif name == "mask_infs":
        program = obs.compile_mask_beyond(R._selection(table, config), None, dtypes)
    elif name == "mask_dewpoint_temperature":
        program = obs.compile_mask_dewpoint(f.temperature, f.dewpoint_temperature, f.specific_humidity if f.mask_specific_humidity else None, dtypes)
    elif name == "exclude_dates":
        program, rows = obs.compile_exclude_dates(f.excluded_dates, dtypes), {obs.DAY_ROW: R.utc_days(table["date"])}
    elif name == "remove_extreme_values":
        names = list(dict.fromkeys(R._selection(table, config) + ["latitude", "longitude"]))
        program = (obs.compile_mask_beyond if f.method == "mask" else obs.compile_keep_not_beyond)(names, f.threshold, dtypes)
    elif name == "clip_tabular":
        program = obs.compile_clip({c: tuple(r) for c, r in f.config.items()}, dtypes)
    elif name == "impute_nans_tabular":
        floats = [c for c in table if dtypes[c].kind == "f" and (not isinstance(f.value, dict) or c in f.value)]
        program = obs.compile_fill_nans({c: (f.value[c] if isinstance(f.value, dict) else f.value) for c in floats}, dtypes)
    else:
        subset = R._selection(table, config) or list(table)
        program = obs.compile_keep_not_missing(subset, f.how, {c: dtypes[c] for c in subset})
        rows = {f"%missing:{c}": R.is_missing(table[c]).astype(np.float64) for c in subset if dtypes[c].kind != "f"}
    return program, rows


def interpreted(name: str, config: dict, table: dict, defect: str | None = None, dtypes_as_float64: bool = False):
    """The statement's answer computed by INTERPRETING the compiled launches: ``("columns", {...})`` in the dtypes the filter hands back,
    or ``("rows", positions)``."""
    seen = {c: (np.asarray(v).astype(np.float64) if dtypes_as_float64 and np.asarray(v).dtype.kind == "f" else v) for c, v in table.items()}
    program, rows = compiled(name, config, seen)
    out = R.run_program(program, table, rows, defect)
    if program.results == (obs.KEEP_ROW,):
        return "rows", np.nonzero(out[obs.KEEP_ROW])[0]
    columns = {}
    for c, row in out.items():
        dtype = np.asarray(table[c]).dtype
        if dtype.kind == "f":
            with np.errstate(over="ignore", invalid="ignore"):
                columns[c] = row.astype(dtype)
        elif name == "clip_tabular":
            columns[c] = row.astype(dtype) if (row == np.floor(row)).all() else row
        else:
            columns[c] = row if np.isnan(row).any() else np.asarray(table[c])
    return "columns", columns


def agree(got, want) -> bool:
    if got[0] != want[0]:
        return False
    if got[0] == "rows":
        return np.array_equal(got[1], want[1])
    changed = {c: v for c, v in want[1].items() if not R.same_bits(v, np.asarray(got[1].get(c, v)))}
    return not changed and set(got[1]) <= set(want[1])


def check_program(program) -> None:
    for launch in program.launches:
        assert 1 <= len(launch.slots) <= R.MAX_OPS == native.MAX_COLUMN_OPS
        for t, slot in enumerate(launch.slots):
            assert slot.src < t and (slot.op not in R.BINARY or t > 0), launch  # every binary slot has a predecessor
            assert (slot.op == "scalar") == (slot.scalar is not None) and (slot.read is None or slot.src < 0)


def case_table(case: dict) -> dict:
    return GOLDEN["tables"][case["table"]]["columns"]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_header_codes_are_the_bindings():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "atx.h")).read()
    assert native.ROW_OPS == R.CODES and set(obs.ROW_BINARY) == R.BINARY
    for name, code in native.ROW_OPS.items():
        assert f"ATX_COLOP_{name.upper()} = {code}" in header
    assert not set(native.ROW_OPS.values()) & set(native.COLUMN_OPS.values()) and min(native.ROW_OPS.values()) == 16
    assert [native.ROW_OPS[f"cmp_{c}"] - 20 for c in ("gt", "lt", "eq", "ne", "ge", "le")] == [native.CMP_GT, native.CMP_LT, native.CMP_EQ,
                                                                                                native.CMP_NE, native.CMP_GE, native.CMP_LE]


def test_argument_checks_of_the_second_family():
    lib = native.load()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first

    def call(ops, srcs, ins=None, outs=None, n=8):
        k = len(ops)
        return lib.atx_obs_column_ops(k, (ctypes.c_int32 * k)(*ops), (ctypes.c_int32 * k)(*srcs), (ctypes.c_void_p * k)(*(ins or [one] * k)),
                                      (ctypes.c_void_p * k)(*(outs or [one] * k)), n, None)

    for code in (10, 15, 33, 64, 96, 98):
        assert call([code], [-1]) == native.EINVAL and b"unknown code" in lib.atx_last_error() and b"operation 0" in lib.atx_last_error()
    assert call([17, 33], [-1, -1]) == native.EINVAL and b"operation 1 has the unknown code 33" in lib.atx_last_error()
    assert call([17, 16], [-1, 0]) == native.EINVAL and b"operation 1 is a SCALAR" in lib.atx_last_error()
    for code in range(20, 33):
        assert call([code], [-1]) == native.EINVAL and b"operation 0" in lib.atx_last_error() and b"binary" in lib.atx_last_error()
    assert call([17, 0], [-1, -1]) == native.EINVAL and b"operation 1" in lib.atx_last_error() and b"mixes the two families" in lib.atx_last_error()
    assert call([0, 17], [-1, -1]) == native.EINVAL and b"mixes the two families" in lib.atx_last_error()
    assert call([17, 20], [-1, 1]) == native.EINVAL and b"not an earlier one" in lib.atx_last_error()
    assert call([18], [-1], ins=[None]) == native.EINVAL and b"null column" in lib.atx_last_error()
    assert call([17] * 17, [-1] * 17) == native.EINVAL and b"1 .. 16" in lib.atx_last_error()
    assert call([16, 20, 29], [-1, -1, -1], ins=[None] * 3, outs=[None] * 3, n=0) == native.OK  # no rows: validated, nothing launched
    assert call([16, 33], [-1, -1], n=0) == native.EINVAL


# ---- the compilers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["id"])
def test_compiled_programs_give_the_statement_on_every_recorded_case(case):
    table = case_table(case)
    program, _ = compiled(case["filter"], case["config"], table)
    check_program(program)
    assert agree(interpreted(case["filter"], case["config"], table), R.statement(case["filter"], case["config"], table)), case["id"]


def test_compiled_programs_give_the_statement_on_random_configurations():
    rng = np.random.default_rng(20261020)
    tables = [R.seeded_table(n) for n in R.SEEDED_ROWS]
    seen = {"launches": 0, "split": 0, "forwarded": 0}
    counts = dict.fromkeys(NINE, 0)
    for k in range(300):
        name, config = R.random_config(rng)
        table = {c: v for c, v in tables[k % 2].items() if c != "label"}
        program, _ = compiled(name, config, table)
        check_program(program)
        assert agree(interpreted(name, config, table), R.statement(name, config, table)), (name, config)
        counts[name] += 1
        seen["launches"] += len(program.launches)
        seen["split"] += len(program.launches) > 1
        seen["forwarded"] += sum(s.src >= 0 for one in program.launches for s in one.slots)
    assert all(counts.values()) and seen["split"] > 10 and seen["forwarded"] > 300, (counts, seen)


def test_an_intermediate_crosses_a_launch_boundary_through_a_row_and_nothing_else_is_stored():
    names = [f"c{k}" for k in range(11)]
    program = obs.compile_keep_not_missing(names, "any", {c: np.dtype("f8") for c in names})
    assert [len(one.slots) for one in program.launches] == [15, 7]
    stores = [[s.store for s in one.slots if s.store] for one in program.launches]
    assert stores == [["%gone"], [obs.KEEP_ROW]] and program.launches[1].slots[1].read == "%gone"
    one = obs.compile_mask_values({"x": ("ge", 0.1)}, {"x": np.dtype("f4")})
    assert one.scalars == (float(np.float32(0.1)),) and [s.op for s in one.launches[0].slots] == ["copy", "scalar", "cmp_ge", "nan_where"]
    assert obs.compile_mask_beyond(["x"], None, {"x": np.dtype("f4")}).scalars == (R.DBL_MAX,)  # not rounded: float32 would make it inf
    with pytest.raises(ValueError, match="numeric"):
        obs.compile_clip({"s": (0, 1)}, {"s": np.dtype("O")})


# ---- the statements against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["id"])
def test_statements_are_the_reference_frames(case):
    table = case_table(case)
    want = R.expected_frame(GOLDEN, case)
    kind, got = R.statement(case["filter"], case["config"], table)
    labels = GOLDEN["tables"][case["table"]]["index"]
    if kind == "rows":
        assert np.array_equal(labels[got], case["index"]) and not case["changed"]
        return
    assert np.array_equal(labels, case["index"])
    for c, column in want.items():
        if column.dtype.kind in "OM" and c in case["changed"]:
            assert case["filter"] in R.FRAME_ONLY  # pandas' own fillna: no statement here
            continue
        assert R.same_bits(got.get(c, table[c]), column), (case["id"], c)


def test_statements_are_pandas_own_on_the_seeded_tables():
    pd = pytest.importorskip("pandas")
    table = {c: v for c, v in R.seeded_table(300).items() if c != "label"}
    df = pd.DataFrame(table)
    _, got = R.statement("mask_tabular", {"b": {"value": 0.1, "operator": ">"}, "i": {"value": 2, "operator": ">="}}, table)
    assert R.same_bits(got["b"], df["b"].mask(df["b"] > 0.1).to_numpy()) and R.same_bits(got["i"], df["i"].mask(df["i"] >= 2).to_numpy())
    _, got = R.statement("clip_tabular", {"b": [0.1, 2.5], "a": [-3.0, None]}, table)
    assert R.same_bits(got["b"], df["b"].clip(0.1, 2.5).to_numpy()) and R.same_bits(got["a"], df["a"].clip(-3.0, None).to_numpy())
    _, rows = R.statement("drop_nans_tabular", {"how": "any", "columns": ["a", "date", "s"]}, table)
    assert np.array_equal(rows, df.dropna(how="any", subset=["a", "date", "s"]).index.to_numpy())
    _, rows = R.statement("remove_extreme_values", {"columns": ["obsvalue_y"], "threshold": 273.15}, table)
    assert np.array_equal(rows, df[~(df[["obsvalue_y", "latitude", "longitude"]].abs() > 273.15).any(axis=1)].index.to_numpy())
    day = R.utc_days(table["date"])
    start, end = pd.to_datetime("20250101", format="%Y%m%d"), pd.to_datetime("20250102", format="%Y%m%d") + pd.Timedelta(days=1)
    assert np.array_equal((day >= R.epoch_day(20250101)) & (day < R.epoch_day(20250102) + 1), ((df["date"] >= start) & (df["date"] < end)).to_numpy())


# ---- the filters on the host double --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["frame", "host"])
def test_filters_give_the_reference_frames_through_the_host_double(monkeypatch, kind):
    pytest.importorskip("pandas")
    R.install_double(monkeypatch)
    for case in GOLDEN["cases"]:
        if kind == "host" and case["filter"] in R.FRAME_ONLY and any(v.dtype.kind == "O" for v in case["changed"].values()):
            with pytest.raises(ValueError, match="not numeric and has missing entries"):
                create_filter_by_name(case["filter"], **case["config"]).forward(R.input_table(GOLDEN, case, kind))
            continue
        table = R.input_table(GOLDEN, case, kind)
        before = R.input_table(GOLDEN, case, kind)
        got = create_filter_by_name(case["filter"], **case["config"]).forward(table)
        assert got is not table
        R.check_case(got, GOLDEN, case, kind)
        for c in before.keys():  # the caller's table is as it was
            assert R.same_column(np.asarray(table[c]), np.asarray(before[c])), (case["id"], c)


# ---- constructors and dispatchers ------------------------------------------------------------------------------------------------------------
def test_registered_and_the_reference_constructor_errors():
    assert set(NINE) <= set(filter_registry.registered)
    for name, config, message in [
        ("mask_tabular", {}, "No columns to mask were specified."),
        ("mask_tabular", {"a": 3}, "Mask condition for column a must be a dictionary"),
        ("mask_tabular", {"a": {"operator": ">"}}, "must contain a 'value' key"),
        ("mask_tabular", {"a": {"value": 1, "operator": "=>"}}, "Invalid operator '=>' for column a. Valid operators are: >, <, ==, !=, >=, <=, gt, lt"),
        ("mask_outside_range", {}, "No columns to mask were specified."),
        ("mask_outside_range", {"a": [1, 2, 3]}, "Invalid mask range for column a"),
        ("mask_outside_range", {"a": ["1", 2]}, "Mask range values for column a must be numeric or None"),
        ("mask_infs", {}, "Either columns or column_prefix must be specified, but not both."),
        ("mask_infs", {"columns": ["a"], "column_prefix": "a"}, "Either columns or column_prefix must be specified, but not both."),
        ("exclude_dates", {}, "No columns to exclude dates from were specified."),
        ("exclude_dates", {"a": 20250101}, "Invalid date ranges 20250101 for column 'a'. Expected a list/tuple."),
        ("exclude_dates", {"a": [[20250101, 20250102, 20250103]]}, "Expected a tuple like"),
        ("remove_extreme_values", {"columns": ["a"], "method": "clip"}, "Invalid method 'clip'. Must be either 'mask' or 'drop'."),
        ("remove_extreme_values", {"method": "mask", "threshold": 1e5}, "Either columns or column_prefix must be specified, but not both."),
        ("remove_extreme_values", {"columns": ["a"], "column_prefix": "a"}, "Either columns or column_prefix must be specified, but not both."),
        ("clip_tabular", {}, "No columns to clip were specified."),
        ("clip_tabular", {"a": 3}, "Invalid clip range for column a"),
        ("clip_tabular", {"a": [None, "x"]}, "Clip range values for column a must be numeric or None"),
        ("impute_nans_tabular", {"value": 0.0, "columns": ["a"], "column_prefix": "a"}, "Either columns or column_prefix may be specified, but not both."),
        ("drop_nans_tabular", {"how": "some"}, "DropNaNs - 'how' must be either 'any' or 'all', not 'some'."),
        ("drop_nans_tabular", {"columns": ["a"], "column_prefix": "a"}, "Either columns or column_prefix may be specified, but not both."),
    ]:
        with pytest.raises(ValueError) as info:
            create_filter_by_name(name, **config)
        assert message in str(info.value), (name, config, str(info.value))


def test_missing_columns_raise_before_any_launch():
    table = {"z": np.array([1.0, np.nan]), "date": np.array(["2025-01-01", "NaT"], dtype="datetime64[ns]")}
    for name, config in [("mask_tabular", {"a": {"value": 1}}), ("mask_outside_range", {"a": [0, 1]}), ("mask_infs", {"columns": ["a"]}),
                         ("mask_infs", {"column_prefix": "obsvalue_"}), ("mask_dewpoint_temperature", {}), ("exclude_dates", {"a": [20250101, 20250101]}),
                         ("remove_extreme_values", {"columns": ["z"]}), ("remove_extreme_values", {"column_prefix": "obsvalue_"}),
                         ("clip_tabular", {"a": [0, 1]}), ("impute_nans_tabular", {"value": 0.0, "columns": ["a"]}),
                         ("impute_nans_tabular", {"value": 0.0, "column_prefix": "obsvalue_"}), ("drop_nans_tabular", {"columns": ["a"]}),
                         ("drop_nans_tabular", {"column_prefix": "obsvalue_"})]:
        with pytest.raises(ValueError, match="missing columns|No columns starting with"):
            create_filter_by_name(name, **config).forward(table)


def test_dispatchers_pick_the_reference_halves():
    from anemoi_transform_amd.fields import FieldList

    mask = create_filter_by_name("mask", a={"value": 2, "operator": ">="})
    assert isinstance(mask.filter, T.MaskValues) and create_filter_by_name("apply_mask", a={"value": 1}).filter.config == {"a": ("==", 1)}
    with pytest.raises(ValueError, match="No columns to mask"):
        create_filter_by_name("mask")
    clip = create_filter_by_name("clip", a=[0, 1])
    assert isinstance(clip.filter, T.ClipTabular) and type(create_filter_by_name("clip", param="t", minimum=0.0).filter).__name__ == "Clipper"
    assert isinstance(create_filter_by_name("clipper", param=[0, 1]).filter, T.ClipTabular)  # a column called param
    with pytest.raises(ValueError, match="No columns to clip"):
        create_filter_by_name("clip")
    both = create_filter_by_name("remove_nans")
    assert isinstance(both.tabular_filter, T.DropNaNsTabular) and both.field_filter is not None
    for config in ({"how": "all"}, {"columns": ["a"]}, {"column_prefix": "a"}):
        f = create_filter_by_name("drop_nans", **config)
        assert isinstance(f.tabular_filter, T.DropNaNsTabular) and f.field_filter is None
        with pytest.raises(ValueError, match="Ambigious config for RemoveNaNs filter."):
            f.forward(FieldList([]))
    fields = create_filter_by_name("remove_nans", param="t")
    assert fields.tabular_filter is None
    with pytest.raises(ValueError, match="Ambigious config for RemoveNaNs filter."):
        fields.forward({"a": np.zeros(2)})
    f = create_filter_by_name("impute_nans", value=0.0, columns=["a"])
    assert isinstance(f.tabular_filter, T.ImputeNaNsTabular) and f.field_filter is None
    with pytest.raises(ValueError, match="Ambiguous config for ImputeNaNs field filter."):
        f.forward(FieldList([]))
    g = create_filter_by_name("replace_nans", param="t", value=0.0)
    assert g.tabular_filter is None
    with pytest.raises(ValueError, match="Ambiguous config for ImputeNans tabular filter."):
        g.forward({"a": np.zeros(2)})
    with pytest.raises(TypeError):
        create_filter_by_name("impute_nans")
    with pytest.raises(TypeError, match="No forward method"):
        mask.forward([1, 2])


def test_dispatchers_run_the_tabular_half_on_a_frame_and_on_a_mapping(monkeypatch):
    pd = pytest.importorskip("pandas")
    R.install_double(monkeypatch)
    columns = {"a": np.array([0.5, np.nan, 3.0, -1.0]), "k": np.array([0, 1, 2, 3])}
    for table in (pd.DataFrame(columns, index=[7, 5, 3, 1]), columns):
        out = create_filter_by_name("mask", k={"value": 2, "operator": ">="}).forward(table)
        assert R.same_bits(np.asarray(out["k"]), np.array([0, 1, np.nan, np.nan])) and R.same_bits(np.asarray(out["a"]), columns["a"])
        out = create_filter_by_name("clip", a=[0.0, 1.0], k=(1, 2)).forward(table)
        assert R.same_bits(np.asarray(out["a"]), np.array([0.5, np.nan, 1.0, 0.0])) and R.same_bits(np.asarray(out["k"]), np.array([1, 1, 2, 2]))
        out = create_filter_by_name("impute_nans", value=9.0, columns=["a"]).forward(table)
        assert R.same_bits(np.asarray(out["a"]), np.array([0.5, 9.0, 3.0, -1.0])) and R.same_bits(np.asarray(out["k"]), columns["k"])
        out = create_filter_by_name("remove_nans", how="any").forward(table)
        assert R.same_bits(np.asarray(out["a"]), np.array([0.5, 3.0, -1.0])) and R.same_bits(np.asarray(out["k"]), np.array([0, 2, 3]))
        assert not hasattr(out, "index") or list(out.index) == [7, 3, 1]
