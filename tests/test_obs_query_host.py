"""``filter_query`` and ``mask_values_custom`` on the host: the query language (parser, numpy's typing, the compiler's order and limits),
the compiled programs through the plain numpy interpreter of tests/row_expr_restatement.py against pandas ITSELF (``DataFrame.query`` /
``eval`` + ``Series.mask``), the two filters against the frames the reference returned (tests/golden/obs_query.json) with the two native
calls answered by that interpreter, the constructor errors, and the declarations and argument checks of ``atx_obs_row_expr`` /
``atx_obs_keep_positions`` through ctypes.  No GPU.  Everything is exact: there is no tolerance in this file.
"""

from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

import row_expr_restatement as X
import row_program_restatement as R
from anemoi_transform_amd import native, query
from anemoi_transform_amd.filters import create_filter_by_name

pd = pytest.importorskip("pandas")
TABLES = X.all_tables()
T48 = TABLES["seeded_48"]["columns"]
DTYPES = {c: v.dtype for c, v in T48.items()}
GOLDEN = X.load_golden()


def _wide() -> dict:
    """The 48-row table with a datetime and a float16 column, which the language refuses."""
    table = dict(T48)
    table["d"] = (np.datetime64("2025-01-01", "ns") + np.arange(48) * np.timedelta64(1, "h")).astype("datetime64[ns]")
    table["h"] = T48["p"].astype(np.float16)
    return table


def _keep(text: str, table: dict = T48) -> np.ndarray:
    return X.run_program(query.compile_query(text, {c: np.asarray(v).dtype for c, v in table.items()}), table)


# ---- parser and compiler -------------------------------------------------------------------------------------------------------------------------
def test_the_two_rewrites_and_the_forms_pandas_reads_the_same():
    same = [("abs(x) > 1 & p < 2", "(abs(x) > 1) and (p < 2)"), ("t | a > 1 & b < 1", "t or ((a > 1) and (b < 1))"), ("`a` > 1 and `p` < 2", "a > 1 and p < 2"),
            ("a == [1, 2]", "a in [1, 2]"), ("a != [1, 2]", "a not in [1, 2]"), ("a in (1, 2)", "a in [1, 2]"), ("~t", "not t"),
            ("s == 'st1'", "s in ['st1']"), ("s != 'st1'", "s not in ['st1']")]
    for text, meaning in same:
        assert query.compile_query(text, DTYPES) == query.compile_query(meaning, DTYPES), text
    # & binds as `and` does, not as Python's &: 1 & p would be an operand of the compare
    assert np.array_equal(_keep("abs(x) > 1 & p < 2"), (np.abs(T48["x"]) > 1) & (T48["p"] < 2))
    # a string literal is left alone by the rewrites
    strings = {"s": np.array(["a&b", "a|b", "`x`", None], dtype=object)}
    assert _keep("s in ['a&b', '`x`']", strings).tolist() == [True, False, True, False]


def test_chained_compares():
    with np.errstate(invalid="ignore"):
        a, p, b = T48["a"], T48["p"], T48["b"]
        assert np.array_equal(_keep("1 < a <= p"), (1 < a) & (a <= p))
        assert np.array_equal(_keep("0.1 <= b < 0.5 <= p"), (np.float32(0.1) <= b) & (b < 0.5) & (0.5 <= p))
        assert np.array_equal(_keep("1 < (a + 1) <= p"), (1 < (a + 1)) & ((a + 1) <= p))
    # a computed middle operand of a three-operand chain is evaluated once: DUP and SWAP, one add
    code = [op for op, *_ in query.compile_query("1 < (a + 1) <= p", DTYPES).code]
    assert code.count("add") == 1 and "dup" in code and "swap" in code


REFUSED = ["@v > 1", "a // 2 > 0", "a % 2 == 0", "a ** 2 > 1", "sqrt(p) > 1", "abs(p, 1) > 1", "(a if t else k) > 1", "p.real > 1", "p[0] > 1",
           "(a in [1, 2]) == k", "1 < a in [2]", "not a", "a and t", "t or p", "t + 1 > 1", "t > 0", "t == t", "t in [1]", "-u < 1", "-(u + u) < 1",
           "d > 0", "d == d", "zz > 1", "a + 1", "p", "h * 2 > 1", "h + h > 1", "s > 1", "s + 1 > 1", "s == 1", "a == 'x'", "a in k", "a in []",
           "a in [1, float('nan')]", "a in [1, 1e999]", "(a + 1) == [1, 2]", "1 < 2", "True", "t == True", "a > 1 and", "a >", "`a > 1", "+a > 1",
           "u - 300 < 0", "a = 1", "lambda: 1", "[a] > 1"]


@pytest.mark.parametrize("text", REFUSED)
def test_refused_constructs_raise_with_the_references_prefixes(monkeypatch, text):
    X.install_double(monkeypatch)
    frame = pd.DataFrame(_wide())
    with pytest.raises(ValueError, match=r"^Invalid query expression: "):
        create_filter_by_name("filter_query", query=text).forward(frame)
    with pytest.raises(ValueError, match=r"^Invalid condition for column 'p': "):
        create_filter_by_name("mask_values_custom", p=text).forward(frame)
    with pytest.raises(ValueError, match=r"^Invalid condition for column 'x': "):  # ... by the name of the condition that is wrong
        create_filter_by_name("mask_values_custom", p="p > 1", x=text).forward(frame)


def test_the_limits_raise_with_their_names():
    deep = "x"
    for _ in range(8):
        deep = f"({deep} + {deep})"  # a complete tree of depth 8 needs 9 slots in any order
    for text, name, size in [(" and ".join(["a > 1"] * 12), "EXPR_MAX_INSTR", 47), (f"a in {list(range(70))}", "EXPR_MAX_CONSTS", 70),
                             (f"{deep} > 1", "EXPR_MAX_STACK", 9)]:
        with pytest.raises(ValueError, match=f"needs {size}, {name} is {getattr(native, name)}"):
            query.compile_query(text, DTYPES)
    with pytest.raises(ValueError, match="needs 5, EXPR_MAX_RESULTS is 4"):
        query.compile_masks([(c, "t") for c in "akubp"], DTYPES)
    assert (native.EXPR_MAX_INPUTS, native.EXPR_MAX_INSTR, native.EXPR_MAX_CONSTS, native.EXPR_MAX_STACK) == (16, 32, 64, 8)
    assert query.compile_query(" and ".join(["a > 1"] * 8), DTYPES).code.__len__() == 31  # ... and just below the limit compiles


def test_sethi_ullman_order_keeps_the_stack_shallow():
    dtypes = {c: v.dtype for c, v in TABLES["seeded_300"]["columns"].items()}
    for text in X.DOCSTRING_QUERIES + tuple(X.DOCSTRING_MASK.values()):
        assert query.compile_query(text, dtypes).depth <= 4, text
    # the deeper operand first: a right-leaning sum needs 2 slots, not 5, and no SWAP (+ commutes); - takes one
    assert query.compile_query("p + (p + (p + (p + x))) > 1", DTYPES).depth == 2
    right = query.compile_query("p - (x * x + p) > 1", DTYPES)
    assert right.depth == 2 and [op for op, *_ in right.code].count("swap") == 1
    with np.errstate(all="ignore"):
        assert np.array_equal(_keep("p - (x * x + p) > 1"), T48["p"] - (T48["x"] * T48["x"] + T48["p"]) > 1)
        assert np.array_equal(_keep("1 > (x * x + p) / p"), 1 > (T48["x"] * T48["x"] + T48["p"]) / T48["p"])


def test_typing_is_numpys():
    ops = lambda text: [op for op, *_ in query.compile_query(text, DTYPES).code]  # noqa: E731
    assert ops("b*a > 0.3").count("round_f32") == 1 and ops("b*p > 0.3").count("round_f32") == 0 and ops("b*k > 0.3").count("round_f32") == 0
    assert ops("b*2 + b > 1").count("round_f32") == 2 and ops("a*2 > 1").count("round_f32") == 0
    # a literal against a float32 operand is rounded to float32; the members of a list are not
    assert query.compile_query("b == 0.1", DTYPES).consts == (float(np.float32(0.1)),)
    assert query.compile_query("b in [0.1]", DTYPES).consts == (0.1,)
    assert query.compile_query("p == 0.1", DTYPES).consts == (0.1,) and query.compile_query("b*0.1 > p", DTYPES).consts == (float(np.float32(0.1)),)
    near = np.flatnonzero(T48["b"] == np.float32(0.1))
    assert len(near) and _keep("b == 0.1")[near].all() and not _keep("b in [0.1]")[near].any()
    nan = np.flatnonzero(np.isnan(T48["p"]))
    assert len(nan) and not _keep("p in [0.0, 1.0]")[nan].any() and _keep("p not in [0.0, 1.0]")[nan].all()


# ---- the compiled program through the restatement, against pandas itself -----------------------------------------------------------------------------
def test_golden_queries_match_pandas():
    for case in X.cases():
        table = TABLES[case["table"]]
        frame = X.frame_of(table)
        if case["filter"] == "filter_query":
            got = _keep(case["config"]["query"], table["columns"])
            assert np.array_equal(got, X.pandas_keep(frame, case["config"]["query"])), case["id"]


def test_random_expressions_match_pandas():
    rng = np.random.default_rng(20261020)
    frame = X.frame_of(TABLES["seeded_48"])
    left_out, seen = 0, set()
    for _ in range(200):
        text = X.random_expression(rng)
        seen.update(op for op, *_ in query.compile_query(text, DTYPES).code)
        try:
            want = X.pandas_keep(frame, text)
        except Exception:  # the generator makes only what pandas and the language both take
            left_out += 1
            continue
        assert np.array_equal(_keep(text), want), text
    assert left_out == 0
    assert seen == set(native.EXPR_OPS) - {"nan_where"}, set(native.EXPR_OPS) - seen


def test_mask_programs_match_pandas(monkeypatch):
    X.install_double(monkeypatch)
    rng = np.random.default_rng(77)
    frame = X.frame_of(TABLES["seeded_48"])
    configs = list(X.MASKS_48) + [{str(c): X.random_expression(rng) for c in rng.choice(list(X.NUMERIC), size=int(rng.integers(1, 4)), replace=False)}
                                  for _ in range(40)]
    for config in configs:
        got = create_filter_by_name("mask_values_custom", **config).forward(frame)
        want = X.pandas_masks(frame, config)
        assert list(got.columns) == list(want.columns) and list(got.index) == list(want.index)
        for c in want.columns:
            assert R.same_column(got[c].to_numpy(), want[c].to_numpy()), (config, c)
    one = query.compile_masks(list(X.MASKS_48[0].items()), DTYPES)  # the second condition takes the first's target from the stack
    assert one.results == ("p", "b") and [op for op, *_ in one.code].count("nan_where") == 2 and "dup" in [op for op, *_ in one.code]
    with pytest.raises(query.SplitNeeded):
        query.compile_masks(list(X.MASKS_48[1].items()), DTYPES)


# ---- against the recorded frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["frame", "host"])
def test_filters_give_the_reference_frames(monkeypatch, kind):
    X.install_double(monkeypatch)
    assert len(GOLDEN["cases"]) == len(X.cases()) >= 29
    for case in GOLDEN["cases"]:
        table = R.input_table(GOLDEN, case, kind)
        kept = {c: np.array(v, copy=True) for c, v in dict(table).items()}
        got = create_filter_by_name(case["filter"], **case["config"]).forward(table)
        assert got is not table, case["id"]
        R.check_case(got, GOLDEN, case, kind)
        for c, v in kept.items():
            assert R.same_column(np.asarray(table[c]), v), (case["id"], c)


def test_the_recorded_file_says_what_the_issue_asks():
    by_id = {case["id"]: case for case in GOLDEN["cases"]}
    assert [int(i) for i in by_id["reference_test_filter_query"]["index"]] == [0, 1]
    masked = by_id["reference_test_mask_values_custom"]
    assert masked["dtypes"]["col1"] == "float64" and R.same_bits(masked["changed"]["col1"], np.array([0.0, 1.0, np.nan, np.nan]))
    assert by_id["seeded_48_mask_3"]["changed"] == {} and by_id["seeded_48_mask_3"]["dtypes"]["k"] == "int64"  # nothing masked: still int64
    assert {c["config"]["query"] for c in GOLDEN["cases"] if c["table"] == "seeded_48" and c["filter"] == "filter_query"} >= {
        "b in [0.1, 0.5]", "b == 0.1", "b*a > 0.3", "b/3 == 0.16666667", "(a*2 - p)/3 >= 0.5", "1 < a <= p", "not (a == 2 or b != b)", "a not in [1, 2]",
        "-b < 1", "t and a > 1", "not t", "abs(a - 3) >= 2"}


# ---- constructors ---------------------------------------------------------------------------------------------------------------------------------
def test_constructor_errors_and_a_missing_column(monkeypatch):
    X.install_double(monkeypatch)
    with pytest.raises(ValueError, match="Query expression cannot be empty"):
        create_filter_by_name("filter_query", query="")
    with pytest.raises(ValueError, match="No columns to mask were specified."):
        create_filter_by_name("mask_values_custom")
    frame = pd.DataFrame({"col2": [3, 4, 5, 6]})
    with pytest.raises(ValueError, match="DataFrame is missing columns: {'col1'}"):
        create_filter_by_name("mask_values_custom", col1="col1 >= 2").forward(frame)
    with pytest.raises(TypeError):
        create_filter_by_name("filter_query", query="a > 1").forward([1, 2, 3])
    empty = create_filter_by_name("filter_query", query="col2 > 4").forward(frame.iloc[:0])
    assert len(empty) == 0 and list(empty.columns) == ["col2"]
    out = create_filter_by_name("filter_query", query="col2 > 4").forward({"col2": np.array([3, 4, 5, 6])})
    assert isinstance(out, dict) and out["col2"].tolist() == [5, 6]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_the_slot_codes_are_gone():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "atx.h")).read()
    for name in ("atx_obs_row_expr", "atx_obs_keep_positions"):
        assert f"ATX_API int {name}(" in header and name in native.SIGNATURES
    assert "filters/tabular/filter_query.py" in header and "filters/tabular/mask_values_custom.py" in header
    for name, code in native.EXPR_OPS.items():  # the codes of the header are the codes of the binding
        assert f"ATX_EXPR_{name.upper()} = {code}" in header
    limits = ("MAX_INPUTS", "MAX_INSTR", "MAX_CONSTS", "MAX_STACK", "MAX_RESULTS", "CHUNK_ROWS")
    for name in limits:
        assert f"#define ATX_EXPR_{name} {getattr(native, 'EXPR_' + name)}\n" in header
    # the slot encoding that carried the program through atx_obs_column_ops is gone: its slot limit, and the five codes, which were
    # the only ATX_COLOP_ names that were defines (the codes of atx_obs_column_ops are enumerators)
    assert sorted(re.findall(r"#define ATX_EXPR_(\w+)", header)) == sorted(limits) and "#define ATX_COLOP_" not in header
    assert not [name for name in vars(native) if name.startswith("COLOP_")]


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = native.load()
    one = ctypes.c_void_p(16).value  # never dereferenced: validation fails first
    EINVAL, OK = native.EINVAL, native.OK
    push, add, in_set = ("push_col", 0), ("add",), native.EXPR_OPS["in_set"]

    def expr(program, inputs, table, outs, n=8, keep=0, words=one, counts=one, **instead):
        """atx_obs_row_expr with the arrays and counts of its arguments, or what ``instead`` names in their place."""
        code = [(native.EXPR_OPS[i[0]] if isinstance(i[0], str) else i[0], *(list(i[1:]) + [0, 0])[:2]) for i in program]
        args = {"n_instr": len(code), "n_inputs": len(inputs), "in": (ctypes.c_void_p * max(len(inputs), 1))(*inputs), "n_consts": len(table),
                "consts": (ctypes.c_double * max(len(table), 1))(*table), "n_results": len(outs), "out": (ctypes.c_void_p * max(len(outs), 1))(*outs)}
        for field, name in enumerate(("code", "arg0", "arg1")):
            args[name] = (ctypes.c_int32 * max(len(code), 1))(*[i[field] for i in code])
        assert set(instead) <= set(args)
        args.update(instead)
        return lib.atx_obs_row_expr(args["n_instr"], args["code"], args["arg0"], args["arg1"], args["n_inputs"], args["in"], args["n_consts"],
                                    args["consts"], args["n_results"], args["out"], keep, words, counts, n, None)

    def refused(status, message):
        said = lib.atx_last_error().decode()
        assert status == EINVAL and said.startswith(("atx_obs_row_expr: ", "atx_obs_keep_positions: ")) and re.search(message, said), (message, said)

    # the malformed programs of tests/test_gpu_obs_query.py::test_argument_errors_reach_python, x and out being `one`
    x = out = one
    bad = [
        ([push] * 33, [x], (), [out], "instructions"), ([push] * 34, [x], (), [out] * 4, "instructions"),
        ([("push_col", k) for k in range(17)], [x] * 17, (), [out], "input columns"), ([push, (in_set, 0, 65)], [x], [0.0] * 65, [out], "constants"),
        ([push] * 5, [x], (), [out] * 5, "value results"), ([push], [x], (), [], "neither"), ([(22, 0, 0)], [x], (), [out], "unknown code"),
        ([push, (-1, 0, 0)], [x], (), [out], "unknown code"), ([push, add], [x], (), [out], "underflow"), ([("swap",)], [x], (), [out], "underflow"),
        ([("dup", 1)], [x], (), [out], "underflow"), ([push] * 9 + [add] * 8, [x], (), [out], "overflow"), ([push, push], [x], (), [out], "leaves 2 values"),
        ([push], [x], (), [out, out], "leaves 1 values"), ([("push_col", 1)], [x], (), [out], "column 1 of 1"), ([("push_col", -1)], [x], (), [out], "column -1"),
        ([("push_const", 2)], [x], [1.0, 2.0], [out], "constant 2 of 2"), ([push, (in_set, 1, 2)], [x], [1.0, 2.0], [out], "IN_SET"),
        ([push, (in_set, 0, 0)], [x], [1.0, 2.0], [out], "IN_SET"), ([push, (in_set, -1, 1)], [x], [1.0, 2.0], [out], "IN_SET"),
        ([push], [None], (), [out], "null input column"), ([push], [x], (), [None], "output row 0 is null"),
    ]
    for code, inputs, consts, outs, message in bad:
        refused(expr(code, inputs, consts, outs), message)
    # what only the flat arguments can say
    for name in ("code", "arg0", "arg1"):
        refused(expr([push], [x], (), [out], **{name: None}), "null program array")
    refused(expr([push], [x], (), [out], n=-1), "-1 rows")
    refused(expr([push], [x], (), [out], n_instr=0), "instructions, got 0")
    for name, message in (("n_inputs", "input columns, got -1"), ("n_consts", "constants, got -1"), ("n_results", "value results, got -1")):
        refused(expr([push], [x], (), [out], **{name: -1}), message)
    refused(expr([("push_const", 0)], [], [1.0], [out], consts=None), "null table")
    refused(expr([push], [x], (), [out], **{"in": None}), "null table")
    refused(expr([push], [x], (), [out], out=None), "null table")
    refused(expr([push], [x], (), [], keep=1, words=None), "null keep_words or chunk_counts")
    refused(expr([push], [x], (), [], keep=1, counts=None), "null keep_words or chunk_counts")
    refused(expr([push], [x], (), [out], keep=1), "leaves 1 values, 1 value results and a keep condition")  # a keep condition needs a slot of its own
    refused(expr([push], [None], (), [None], keep=1, n=0, words=None, counts=None), "leaves 1 values")  # ... without rows too: keep is a flag
    # no rows: validated, nothing launched, whatever the rows are
    assert expr([push], [None], (), [None], n=0) == OK
    assert expr([push], [None], (), [], n=0, keep=1, words=None, counts=None) == OK
    assert expr([push, ("push_const", 0), ("cmp_gt",)], [None], [1.0], [], n=0, keep=1, words=None, counts=None) == OK

    # atx_obs_keep_positions(keep_words, chunk_offsets, n, positions, n_positions, stream)
    refused(lib.atx_obs_keep_positions(one, one, -1, one, 1, None), "-1 rows")
    refused(lib.atx_obs_keep_positions(one, one, 8, one, -1, None), "-1 positions")
    for words, offsets, positions in ((None, one, one), (one, None, one), (one, one, None)):
        refused(lib.atx_obs_keep_positions(words, offsets, 8, positions, 1, None), "null pointer")
    assert lib.atx_obs_keep_positions(None, None, 0, None, 1, None) == OK
    assert lib.atx_obs_keep_positions(None, None, 8, None, 0, None) == OK
