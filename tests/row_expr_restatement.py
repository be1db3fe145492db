"""The row-expression programs of ``filter_query`` and ``mask_values_custom``, restated without the package: a plain numpy interpreter of
the row-expression kernel's instruction set (include/atx.h: a postfix program, a stack, float64 rows; ``astype(float32).astype(float64)`` for
``ROUND_F32``), the packing of keep bits into words and chunk counts, pandas itself as the oracle (``DataFrame.query`` / ``eval`` +
``Series.mask``), the tables and cases that ``tools/record_obs_query_golden.py`` ran through the reference's own ``forward``
(tests/golden/obs_query.json), and a generator of random typed expressions.

A helper, not a test file.  Used by tests/test_obs_query_host.py and tests/test_gpu_obs_query.py.
"""

from __future__ import annotations

import json
import os
import warnings

import numpy as np

import row_program_restatement as R
from rowset_restatement import decode, encode, same_bits  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obs_query.json")
CODES = {"push_col": 0, "push_const": 1, "add": 2, "sub": 3, "mul": 4, "div": 5, "neg": 6, "abs": 7, "round_f32": 8, "cmp_gt": 9, "cmp_lt": 10,
         "cmp_eq": 11, "cmp_ne": 12, "cmp_ge": 13, "cmp_le": 14, "in_set": 15, "and": 16, "or": 17, "not": 18, "dup": 19, "swap": 20,
         "nan_where": 21}
NAMES = {code: name for name, code in CODES.items()}
MAX_INPUTS, MAX_INSTR, MAX_CONSTS, MAX_STACK, MAX_RESULTS, CHUNK_ROWS = 16, 32, 64, 8, 4, 256
QUIET_NAN = R.QUIET_NAN
SIGN = np.uint64(1 << 63)


# ---- the interpreter -----------------------------------------------------------------------------------------------------------------------
def _flag(c: np.ndarray) -> np.ndarray:
    return np.where(c, 1.0, 0.0)


def run(code, inputs, consts, n: int) -> list[np.ndarray]:
    """The stack a program leaves, bottom first: ``code`` is a list of ``(code, arg0, arg1)`` with integer codes, ``inputs`` float64 arrays
    of ``n``, ``consts`` floats.  NEG, ABS and the selects work on bits, everything else is numpy's float64 arithmetic."""
    assert 1 <= len(code) <= MAX_INSTR and len(inputs) <= MAX_INPUTS and len(consts) <= MAX_CONSTS
    consts = np.asarray(consts, dtype=np.float64)
    stack: list[np.ndarray] = []
    with np.errstate(all="ignore"):
        for op, a, b in code:
            name = NAMES[int(op)]
            if name == "push_col":
                stack.append(np.array(inputs[a], dtype=np.float64, copy=True))
            elif name == "push_const":
                stack.append(np.full(n, consts[a]))
            elif name == "dup":
                stack.append(stack[-1 - a].copy())
            elif name == "swap":
                stack[-1], stack[-2] = stack[-2], stack[-1]
            elif name == "neg":
                stack[-1] = (stack[-1].view(np.uint64) ^ SIGN).view(np.float64)
            elif name == "abs":
                stack[-1] = (stack[-1].view(np.uint64) & ~SIGN).view(np.float64)
            elif name == "round_f32":
                stack[-1] = stack[-1].astype(np.float32).astype(np.float64)
            elif name == "not":
                stack[-1] = _flag(stack[-1] == 0)
            elif name == "in_set":
                assert b >= 1 and a + b <= len(consts)
                stack[-1] = _flag(np.logical_or.reduce([stack[-1] == v for v in consts[a:a + b]]))
            else:
                y = stack.pop()
                x = stack.pop()
                stack.append({"add": lambda: x + y, "sub": lambda: x - y, "mul": lambda: x * y, "div": lambda: x / y,
                              "cmp_gt": lambda: _flag(x > y), "cmp_lt": lambda: _flag(x < y), "cmp_eq": lambda: _flag(x == y),
                              "cmp_ne": lambda: _flag(x != y), "cmp_ge": lambda: _flag(x >= y), "cmp_le": lambda: _flag(x <= y),
                              "and": lambda: _flag((x != 0) & (y != 0)), "or": lambda: _flag((x != 0) | (y != 0)),
                              "nan_where": lambda: np.where(y != 0, QUIET_NAN, x)}[name]())
            assert len(stack) <= MAX_STACK
    return stack


def pack_words(keep: np.ndarray) -> np.ndarray:
    """A bool row as ``ceil(n / 64)`` uint64 words, bit ``row % 64`` of word ``row / 64``; the padding bits are 0."""
    keep = np.asarray(keep, dtype=bool)
    padded = np.zeros((len(keep) + 63) // 64 * 64, dtype=bool)
    padded[:len(keep)] = keep
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def chunk_counts(keep: np.ndarray) -> np.ndarray:
    keep = np.asarray(keep, dtype=bool)
    padded = np.zeros((len(keep) + CHUNK_ROWS - 1) // CHUNK_ROWS * CHUNK_ROWS, dtype=np.uint8)
    padded[:len(keep)] = keep
    return padded.reshape(-1, CHUNK_ROWS).sum(axis=1, dtype=np.int64)


def string_leaf(leaf, column) -> np.ndarray:
    values = np.asarray(column, dtype=object).tolist()
    hit = np.array([isinstance(v, str) and v in leaf.values for v in values], dtype=bool)
    return ~hit if leaf.op == "not in" else hit


def run_program(program, table: dict):
    """An ``ExprProgram`` (anything with ``inputs``, ``code`` of named operations, ``consts``, ``results``, ``keep``, ``host``) over a table of
    numpy columns: the bool keep row, or ``{name: float64 row}`` of its value results."""
    inputs = []
    for name in program.inputs:
        if name.startswith("%host:"):
            leaf = program.host[int(name[6:])]
            inputs.append(string_leaf(leaf, table[leaf.column]).astype(np.float64))
        else:
            inputs.append(np.asarray(table[name]).astype(np.float64))
    n = len(next(iter(table.values())))
    stack = run([(CODES[op], a, b) for op, a, b in program.code], inputs, program.consts, n)
    assert len(stack) == len(program.results) + (1 if program.keep else 0)
    return stack[-1] != 0 if program.keep else dict(zip(program.results, stack))


def install_double(monkeypatch) -> None:
    """``native.obs_row_expr`` / ``obs_keep_positions`` answered by this file on host tensors, and this process's device the host: the
    Python layers of the two filters run where there is no GPU."""
    import torch

    from anemoi_transform_amd import native, stack

    def obs_row_expr(instructions, inputs, consts, outs, n, keep_words=None, chunk_counts=None):
        left = run(list(instructions), [t.numpy() for t in inputs], consts, n)
        assert len(left) == len(outs) + (keep_words is not None)
        for out, row in zip(outs, left):
            out.numpy()[:] = row
        if keep_words is not None:
            keep_words.numpy()[:] = pack_words(left[-1] != 0).view(np.int64)
            chunk_counts.numpy()[:] = globals()["chunk_counts"](left[-1] != 0)

    def obs_keep_positions(keep_words, chunk_offsets, n, positions):
        bits = np.unpackbits(keep_words.numpy().view(np.uint8), bitorder="little")[:n]
        positions.numpy()[:] = np.flatnonzero(bits)

    monkeypatch.setattr(native, "obs_row_expr", obs_row_expr)
    monkeypatch.setattr(native, "obs_keep_positions", obs_keep_positions)
    monkeypatch.setattr(stack, "device", lambda: torch.device("cpu"))


# ---- pandas itself --------------------------------------------------------------------------------------------------------------------------
def pandas_keep(frame, text: str) -> np.ndarray:
    """The rows ``frame.query(text)`` keeps, as a bool row (the frame's index is unique)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = frame.query(text)
    return np.asarray(frame.index.isin(out.index))


def pandas_masks(frame, config: dict):
    """``mask_values_custom``'s statement on a copy: per condition, in order, ``eval`` and ``Series.mask``."""
    frame = frame.copy(deep=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for col, text in config.items():
            frame[col] = frame[col].mask(frame.eval(text))
    return frame


# ---- tables and cases ------------------------------------------------------------------------------------------------------------------------
LITERALS = (0.1, 0.5, 0.3, 0.16666667, 1.0, 2.0, 3.0)
DOCSTRING_QUERIES = ("varno in [1,2,3,4,7,59] and pressure in [85000, 92500, 100000]",
                     "abs(fg_depar_t_0) < 15 and pressure > 50000 and abs(latitude) < 80",
                     "(varno == 2 and abs(fg_depar_t_0) < 15) or (varno == 7 and abs(fg_depar_q_0) < 0.005)")
DOCSTRING_MASK = {"fg_depar_z_0": "abs(fg_depar_z_0) > 500 & pressure < 50000"}
QUERIES_48 = ("b in [0.1, 0.5]", "b == 0.1", "b*a > 0.3", "b/3 == 0.16666667", "(a*2 - p)/3 >= 0.5", "1 < a <= p", "not (a == 2 or b != b)",
              "a not in [1, 2]", "-b < 1", "t and a > 1", "not t", "abs(a - 3) >= 2", "1 < (a + u) <= k", "x != [0.0, 0.5] | `k` == [3]",
              "b + x*b - b/a >= p", "s in ['st1', 'st3'] and a > 0", "s != 'st2' & t", "0.1 <= b < 0.5 <= p", "u*b in [0.5, 1.0, 1.5]")
MASKS_48 = ({"p": "p > 2 & a > 1", "b": "p != p | b < 0"},           # the second condition reads the first's target
            {"a": "a >= 2", "x": "a != a and t"},                      # ... an INTEGER target: one launch per condition
            {"b": "b*a > 0.3", "x": "abs(x) > 1 | s == 'st1'", "k": "k in [1, 2]", "u": "not t"},
            {"k": "k > 100"})                                          # nothing masked: the integer column comes back as it is


def reference_tables() -> dict:
    """R: tests/tabular_filters/test_filter_query.py and test_mask_values_custom.py, their frames."""
    strings = np.empty(5, dtype=object)
    strings[:] = ["a", "b", "a", "d", "e"]
    return {"reference_query": {"col1": np.array([1, 2, 3, 2, 1]), "col2": strings, "col3": np.array([0, 1, 2, 3, 4])},
            "reference_two_columns": {"col1": np.array([0, 1, 2, 3]), "col2": np.array([3, 4, 5, 6])}}


def _beside(value: float) -> list[float]:
    f = np.float32(value)
    return [value, float(f), float(np.nextafter(f, np.float32(np.inf))), float(np.nextafter(f, np.float32(-np.inf)))]


def table_48() -> dict:
    """48 rows: ``a`` int16, ``k`` int64, ``u`` uint8, ``b`` float32, ``p`` / ``x`` float64, ``t`` bool, ``s`` strings with None; ``label``: the
    DataFrame's index labels.  The float columns run through NaN, +-inf, +-0.0, float32 subnormals and every literal of the queries
    with one float32 ulp either side; the integers are small (nothing wraps in numpy)."""
    rng = np.random.default_rng(4800)
    n = 48
    pool = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -3e-45, 1.1754942e-38, 5e-324]
    for v in LITERALS:
        pool += _beside(v)
    pool = np.array(pool, dtype=np.float64)

    def floats():
        v = np.round(rng.standard_normal(n) * 2.0, 2)
        at = rng.permutation(n)[:len(pool)]
        v[at] = pool[:len(at)]
        return v

    with np.errstate(over="ignore", under="ignore"):
        table = {"a": rng.integers(-5, 9, n).astype(np.int16), "k": rng.integers(-3, 7, n).astype(np.int64), "u": rng.integers(0, 4, n).astype(np.uint8),
                 "b": floats().astype(np.float32), "p": floats(), "x": np.where(rng.random(n) < 0.5, floats(), rng.choice([0.0, 0.5, 1.0, 2.0], n)),
                 "t": rng.random(n) < 0.5}
    s = np.empty(n, dtype=object)
    s[:] = [None if rng.random() < 0.15 else f"st{int(v)}" for v in rng.integers(0, 5, n)]
    table["s"] = s
    table["label"] = (500 + 3 * rng.permutation(n)).astype(np.int64)
    return table


def table_300() -> dict:
    """300 rows with the column names of the reference's docstrings."""
    rng = np.random.default_rng(30000)
    n = 300
    table = {"varno": rng.choice([1, 2, 3, 4, 7, 29, 59, 111], n).astype(np.int64),
             "pressure": rng.choice([100000.0, 92500.0, 85000.0, 70000.0, 50000.0, 49999.99, 30000.0, np.nan], n),
             "fg_depar_t_0": np.where(rng.random(n) < 0.1, np.nan, np.round(rng.standard_normal(n) * 12.0, 3)),
             "fg_depar_q_0": np.where(rng.random(n) < 0.1, np.nan, rng.standard_normal(n) * 0.004),
             "fg_depar_z_0": np.where(rng.random(n) < 0.1, np.nan, np.round(rng.standard_normal(n) * 400.0, 1)),
             "latitude": rng.uniform(-90, 90, n), "longitude": rng.uniform(-180, 180, n)}
    table["fg_depar_t_0"][:4] = [15.0, -15.0, 14.999999999999998, np.inf]
    table["fg_depar_z_0"][:4] = [500.0, -500.0, 500.00000000000006, -np.inf]
    table["latitude"][:3] = [80.0, -80.0, 79.99999999999999]
    table["label"] = (9000 + 11 * rng.permutation(n)).astype(np.int64)
    return table


SEEDED = {"seeded_48": table_48, "seeded_300": table_300}


def cases() -> list[dict]:
    out = [dict(id="reference_test_filter_query", filter="filter_query", config={"query": "col1 in [1,2] and col2 in ['a', 'b']"},
                table="reference_query", kept_index=[0, 1]),
           dict(id="reference_test_mask_values_custom", filter="mask_values_custom", config={"col1": "col1 >= 2"}, table="reference_two_columns",
                literals={"col1": [0, 1, float("nan"), float("nan")]})]
    out += [dict(id=f"docstring_query_{k}", filter="filter_query", config={"query": q}, table="seeded_300") for k, q in enumerate(DOCSTRING_QUERIES)]
    out.append(dict(id="docstring_mask", filter="mask_values_custom", config=dict(DOCSTRING_MASK), table="seeded_300"))
    out += [dict(id=f"seeded_48_query_{k:02d}", filter="filter_query", config={"query": q}, table="seeded_48") for k, q in enumerate(QUERIES_48)]
    out += [dict(id=f"seeded_48_mask_{k}", filter="mask_values_custom", config=dict(m), table="seeded_48") for k, m in enumerate(MASKS_48)]
    return out


def all_tables() -> dict:
    """``{name: {"index": labels, "columns": {...}}}`` of every table the cases use."""
    tables = {name: {"index": np.arange(len(next(iter(cols.values()))), dtype=np.int64), "columns": cols} for name, cols in reference_tables().items()}
    for name, make in SEEDED.items():
        cols = make()
        tables[name] = {"index": cols.pop("label"), "columns": cols}
    return tables


def frame_of(table: dict):
    import pandas as pd

    return pd.DataFrame(dict(table["columns"]), index=table["index"])


# ---- the golden file --------------------------------------------------------------------------------------------------------------------------
def load_golden() -> dict:
    """As ``row_program_restatement.load_golden``: ``{"tables": ..., "cases": [...]}``, a case with ``index`` (the labels that came out),
    ``changed`` (decoded columns), ``dtypes`` (of every column that came out) and ``digest``; its checkers (``R.expected_frame``,
    ``R.input_table``, ``R.check_case``) read the result.  The tables are made here and must have the recorded digests."""
    with open(GOLDEN) as f:
        raw = json.load(f)
    tables = all_tables()
    for name, t in tables.items():
        assert R.frame_digest(t["columns"]) == raw["tables"][name]["digest"], name
    out = []
    for case in raw["cases"]:
        table = tables[case["table"]]
        n = len(table["index"])
        rows = np.flatnonzero(~R.unpack_rows(case["dropped"], n)) if "dropped" in case else np.arange(n)
        case = {key: value for key, value in case.items() if key != "dropped"}
        case["index"] = table["index"][rows]
        case["changed"] = {c: R.unpack_changed(table["columns"][c][rows], record) for c, record in case["changed"].items()}
        case["dtypes"] = {c: case["dtypes"].get(c, str(v.dtype)) for c, v in table["columns"].items()}
        out.append(case)
    return {"tables": tables, "cases": out}


# ---- random typed expressions over table_48 ---------------------------------------------------------------------------------------------------
NUMERIC = {"a": np.dtype(np.int16), "k": np.dtype(np.int64), "u": np.dtype(np.uint8), "b": np.dtype(np.float32), "p": np.dtype(np.float64),
           "x": np.dtype(np.float64)}
INT_LITERALS = (0, 1, 2, 3, 4)
FLOAT_LITERALS = (0.1, 0.5, 0.3, 0.16666667, 1.0, 2.5, -0.5, 1e-40)


def _literal(rng, integers_only: bool = False):
    if integers_only or rng.random() < 0.5:
        return int(rng.choice(INT_LITERALS))
    return float(rng.choice(FLOAT_LITERALS))


def _numeric(rng, depth: int):
    """``(text, dtype or a Python literal)``: only what the language takes and only where numpy does not wrap an integer — at most two
    levels of arithmetic over small integers, no subtraction that stays unsigned, no negation of an unsigned operand."""
    if depth == 0 or rng.random() < 0.3:
        name = str(rng.choice(list(NUMERIC)))
        return (f"`{name}`" if rng.random() < 0.1 else name), NUMERIC[name]
    kind = rng.random()
    x, tx = _numeric(rng, depth - 1)
    if kind < 0.12 and np.dtype(tx).kind != "u":
        return f"(-{x})", tx
    if kind < 0.24:
        return f"abs({x})", tx
    if rng.random() < 0.4:
        y, ty = _literal(rng), None
        y_text = repr(y)
    else:
        y_text, ty = _numeric(rng, depth - 1)
        y = None
    op = str(rng.choice(["+", "-", "*", "/"]))
    result = np.result_type(tx, y if ty is None else ty)
    if op == "-" and result.kind == "u":
        op = "+"
    if op == "/" and result.kind in "iu":
        result = np.dtype(np.float64)
    if ty is None and rng.random() < 0.5 and op in "+*":
        return f"({y_text} {op} {x})", result
    return f"({x} {op} {y_text})", result


def _condition(rng, depth: int) -> str:
    kind = rng.random()
    if depth > 0 and kind < 0.35:
        op = str(rng.choice(["and", "or", "&", "|"]))
        return f"({_condition(rng, depth - 1)}) {op} ({_condition(rng, depth - 1)})"
    if depth > 0 and kind < 0.45:
        return f"not ({_condition(rng, depth - 1)})"
    if kind < 0.5:
        return "t"
    if kind < 0.55:
        values = [f"'st{int(v)}'" for v in rng.integers(0, 6, int(rng.integers(1, 4)))]
        form = rng.random()
        if form < 0.25:
            return f"s == {values[0]}"
        if form < 0.5:
            return f"s != {values[0]}"
        return f"s {'in' if form < 0.75 else 'not in'} [{', '.join(values)}]"
    x, _ = _numeric(rng, 2)
    if kind < 0.7:
        members = ", ".join(repr(_literal(rng)) for _ in range(int(rng.integers(1, 5))))
        if rng.random() < 0.3:  # pandas reads == [..] as membership for a plain column only
            return f"{rng.choice(list(NUMERIC))} {rng.choice(['==', '!='])} [{members}]"
        return f"{x} {rng.choice(['in', 'not in'])} [{members}]"
    compare = lambda: str(rng.choice(["<", "<=", ">", ">=", "==", "!="]))  # noqa: E731
    if kind < 0.8:
        y, _ = _numeric(rng, 1)
        z = repr(_literal(rng)) if rng.random() < 0.5 else _numeric(rng, 1)[0]
        return f"{x} {compare()} {y} {compare()} {z}"
    y = repr(_literal(rng)) if rng.random() < 0.6 else _numeric(rng, 2)[0]
    return f"{y} {compare()} {x}" if rng.random() < 0.2 else f"{x} {compare()} {y}"


def _cost(text: str) -> int:
    """An upper bound of the instructions the expression compiles to: a token each, a SWAP for every - and /, ``+ 0.0`` for every *, DUP SWAP AND for every
    compare (as if each were chained)."""
    import re

    tokens = re.findall(r"[A-Za-z_][A-Za-z_0-9]*|'[^']*'|\d[\d.e-]*|<=|>=|==|!=|[-+*/<>&|]", text)
    return len(tokens) + sum(t in "-/" for t in tokens) + 2 * tokens.count("*") + 3 * sum(t in ("<", "<=", ">", ">=", "==", "!=") for t in tokens)


def random_expression(rng: np.random.Generator) -> str:
    """One expression in the language, over ``table_48``'s columns, that fits one launch (the generator draws again until ``_cost`` says so)."""
    while True:
        text = _condition(rng, 2)
        if _cost(text) <= MAX_INSTR:
            return text
