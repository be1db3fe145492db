"""The query language of ``filter_query`` and ``mask_values_custom``: pandas' ``DataFrame.query`` / ``eval`` expressions, parsed on the host
and compiled to a postfix program for the row-expression kernel (csrc/atx_obs_row_expr.hip; ``native.obs_row_expr``).

The text is parsed with Python's ``ast`` after the two rewrites pandas' own ``pandas`` parser makes: ``&`` / ``|`` become ``and`` / ``or``
with THEIR precedence (``abs(x) > 500 & p < 50000`` is a conjunction of two compares), and a backtick-quoted name is a column name.

Accepted: column names, int and float literals; ``+ - * /``, unary ``-``, ``abs(...)``; ``< <= > >= == !=``, chained; ``x in [..]``, ``x not
in [..]``, ``x == [..]``, ``x != [..]`` with a list of finite numbers; ``and or not`` on boolean operands; ``<string column> == | != | in |
not in <string literal(s)>`` as a leaf evaluated on the host.  Everything else raises ``ValueError``.

TYPING FOLLOWS NUMPY, because pandas' python engine is numpy.  Every arithmetic node has the dtype ``np.result_type`` gives its operands;
a literal enters as a Python scalar, which is weak (NEP 50).  A float32 node is evaluated in float64 and rounded by ``ROUND_F32`` — for ``+ -
* /`` of float32 operands that double rounding is innocuous (53 >= 2 * 24 + 2) — and a literal operand of it is rounded to float32
first, as numpy converts it.  A float16 node is refused.  Integer columns ride in float64: exact below 2^53; where numpy would wrap a
narrow integer, the result here is the mathematical value (documented, not handled); an integer product or negation never yields
``-0.0`` (the product is followed by ``+ 0.0``, the negation is ``0 - x``), since ``1 / (k * 0)`` is ``+inf`` in numpy whatever the sign of k.  A literal compared with a float32 / float16
operand is rounded to that precision (``b == 0.1`` is true for a float32 0.1); the members of an ``in`` list are NOT (pandas' ``isin``
compares in float64: ``b in [0.1]`` is false for it).  A NaN is in no list.

The compiler emits operands in Sethi-Ullman order (the operand that needs the deeper stack first), so the evaluation stack stays
shallow.  The limits are ``native.EXPR_MAX_*``; an expression beyond one raises ``ValueError`` naming the limit and the size.
"""

from __future__ import annotations

import ast
import math
from typing import Any, Mapping, NamedTuple, Sequence

import numpy as np
import torch

from . import native

HOST_ROW = "%host:"  # the 0 / 1 input row of a string leaf, evaluated on the host
BOOL = "bool"
_ARITH = {ast.Add: "add", ast.Sub: "sub", ast.Mult: "mul", ast.Div: "div"}
_COMPARE = {ast.Gt: "cmp_gt", ast.Lt: "cmp_lt", ast.Eq: "cmp_eq", ast.NotEq: "cmp_ne", ast.GtE: "cmp_ge", ast.LtE: "cmp_le"}
_FLIPPED = {"cmp_gt": "cmp_lt", "cmp_lt": "cmp_gt", "cmp_ge": "cmp_le", "cmp_le": "cmp_ge", "cmp_eq": "cmp_eq", "cmp_ne": "cmp_ne"}
_COMMUTATIVE = {"add", "mul", "and", "or", "cmp_eq", "cmp_ne"}
_PYTHON = {"add": lambda x, y: x + y, "sub": lambda x, y: x - y, "mul": lambda x, y: x * y, "div": lambda x, y: x / y}


class HostLeaf(NamedTuple):
    """``column OP values`` on a string column: ``op`` is ``"in"`` or ``"not in"`` (``==`` / ``!=`` with one value are those)."""
    column: str
    op: str
    values: tuple[str, ...]


class ExprProgram(NamedTuple):
    """One launch of the row-expression kernel (``native.obs_row_expr``).  ``inputs``: the rows it reads, column names or ``%host:<k>`` (the 0 / 1 row of ``host[k]``);
    ``code``: ``(operation, arg0, arg1)`` in postfix order, operation a ``native.EXPR_OPS`` name; ``consts``: the constant table;
    ``results``: the columns whose new values the stack slots 0 .. hold when the program ends; ``keep``: one more slot on top of them is
    the keep condition; ``depth``: the deepest the stack gets."""
    inputs: tuple[str, ...]
    code: tuple[tuple[str, int, int], ...]
    consts: tuple[float, ...]
    results: tuple[str, ...]
    keep: bool
    host: tuple[HostLeaf, ...]
    depth: int


class SplitNeeded(ValueError):
    """Conditions that cannot share one program: each one compiles, the caller runs them one launch each."""


# ---- the two rewrites ---------------------------------------------------------------------------------------------------------------------
def rewrite(text: str) -> tuple[str, dict[str, str]]:
    """``&`` -> ``and``, ``|`` -> ``or`` and `` `name` `` -> a placeholder identifier, outside string literals.  Returns the new text and
    placeholder -> column name."""
    out, names, i, n = [], {}, 0, len(text)
    while i < n:
        c = text[i]
        if c in "'\"":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1])
            i = j + 1
        elif c == "`":
            j = text.find("`", i + 1)
            if j < 0:
                raise ValueError("unterminated backtick-quoted name")
            key = f"_atx_backtick_{len(names)}_"
            names[key] = text[i + 1:j]
            out.append(f" {key} ")
            i = j + 1
        elif c in "&|":
            out.append(" and " if c == "&" else " or ")
            i += 1
        else:
            out.append(c)
            i += 1
    return "".join(out), names


# ---- the typed tree -----------------------------------------------------------------------------------------------------------------------
class Node(NamedTuple):
    """``kind``: ``col`` (value: name), ``const`` (value: a Python number, weak), ``un`` / ``bin`` (value: operation), ``in`` (value: (members,
    negate)), ``chain`` (value: (op1, op2); args: first, middle, last), ``host`` (value: index).  ``ty``: a numpy dtype, None for a
    literal, ``BOOL`` for a condition."""
    kind: str
    value: Any
    args: tuple
    ty: Any


def _kind(dtype: Any) -> str:
    if isinstance(dtype, torch.dtype):
        if dtype == torch.bool:
            return "b"
        return "f" if dtype.is_floating_point else ("c" if dtype.is_complex else ("u" if str(dtype).startswith("torch.uint") else "i"))
    return np.dtype(dtype).kind


def _numpy_dtype(dtype: Any) -> np.dtype:
    return torch.empty(0, dtype=dtype).numpy().dtype if isinstance(dtype, torch.dtype) else np.dtype(dtype)


class _Typer:
    def __init__(self, dtypes: Mapping[str, Any], backticks: Mapping[str, str], host: list[HostLeaf]) -> None:
        self.dtypes, self.backticks, self.host = dtypes, backticks, host

    def column(self, node: ast.Name) -> tuple[str, str]:
        name = self.backticks.get(node.id, node.id)
        if name not in self.dtypes:
            raise ValueError(f"name '{name}' is not defined: no such column")
        return name, _kind(self.dtypes[name])

    def numeric(self, node: ast.AST, what: str) -> Node:
        out = self.visit(node)
        if out.ty == BOOL:
            raise ValueError(f"{what} needs a numeric operand, got a boolean one")
        return out

    def boolean(self, node: ast.AST, what: str) -> Node:
        out = self.visit(node)
        if out.ty != BOOL:
            raise ValueError(f"'{what}' needs a boolean operand, got a numeric one")
        return out

    def visit(self, node: ast.AST) -> Node:
        if isinstance(node, ast.Name):
            name, kind = self.column(node)
            if kind in "Mm":
                raise ValueError(f"column '{name}' holds datetimes, which a query cannot use here")
            if kind == "b":
                return Node("col", name, (), BOOL)
            if kind not in "iuf":
                raise ValueError(f"column '{name}' is not numeric: only '{name} == | != | in | not in <string literal(s)>' is taken")
            return Node("col", name, (), _numpy_dtype(self.dtypes[name]))
        if isinstance(node, ast.Constant):
            if isinstance(node.value, bool) or not isinstance(node.value, (int, float)):
                raise ValueError(f"the literal {node.value!r} is not taken here: int and float literals only")
            return Node("const", node.value, (), None)
        if isinstance(node, ast.BinOp):
            if type(node.op) not in _ARITH:
                raise ValueError(f"the operator {type(node.op).__name__} is not taken: + - * / only")
            return self.arith(_ARITH[type(node.op)], self.numeric(node.left, "arithmetic"), self.numeric(node.right, "arithmetic"))
        if isinstance(node, ast.UnaryOp):
            if isinstance(node.op, (ast.Not, ast.Invert)):
                return Node("un", "not", (self.boolean(node.operand, "not"),), BOOL)
            if not isinstance(node.op, ast.USub):
                raise ValueError(f"the unary operator {type(node.op).__name__} is not taken")
            x = self.numeric(node.operand, "unary minus")
            if x.kind == "const":
                return Node("const", -x.value, (), None)
            if x.ty.kind == "u":
                raise ValueError(f"unary minus on an unsigned operand of dtype {x.ty}")
            if x.ty.kind == "i":  # an integer zero has no sign: 0 - x, not a flipped sign bit
                return Node("bin", "sub", (Node("const", 0.0, (), None), x), x.ty)
            return Node("un", "neg", (x,), x.ty)
        if isinstance(node, ast.Call):
            if not (isinstance(node.func, ast.Name) and node.func.id == "abs" and len(node.args) == 1 and not node.keywords):
                raise ValueError("the only function taken is abs(x)")
            x = self.numeric(node.args[0], "abs")
            return Node("const", abs(x.value), (), None) if x.kind == "const" else Node("un", "abs", (x,), x.ty)
        if isinstance(node, ast.BoolOp):
            name = "and" if isinstance(node.op, ast.And) else "or"
            args = [self.boolean(v, name) for v in node.values]
            out = args[0]
            for right in args[1:]:
                out = Node("bin", name, (out, right), BOOL)
            return out
        if isinstance(node, ast.Compare):
            return self.compare(node)
        raise ValueError(f"'{type(node).__name__}' nodes are not taken")

    def arith(self, op: str, x: Node, y: Node) -> Node:
        if x.kind == "const" and y.kind == "const":
            try:
                return Node("const", _PYTHON[op](x.value, y.value), (), None)
            except (ZeroDivisionError, OverflowError) as e:
                raise ValueError(f"{x.value} {op} {y.value}: {e}") from None
        try:
            ty = np.result_type(*(a.value if a.kind == "const" else a.ty for a in (x, y)))
        except OverflowError as e:
            raise ValueError(str(e)) from None
        if ty.kind in "iu":
            for a in (x, y):
                if a.kind == "const" and not np.iinfo(ty).min <= a.value <= np.iinfo(ty).max:
                    raise ValueError(f"Python integer {a.value} out of bounds for {ty}")
            if op == "div":
                ty = np.dtype(np.float64)
        if ty == np.float16:
            raise ValueError("an operation whose result is float16 is not taken")
        if ty.kind != "f" and ty.kind not in "iu":
            raise ValueError(f"an operation whose result is {ty} is not taken")
        if ty == np.float32:  # numpy converts a weak literal to float32 before it computes
            with np.errstate(over="ignore"):
                x, y = (Node("const", float(np.float32(a.value)), (), None) if a.kind == "const" else a for a in (x, y))
            return Node("un", "round_f32", (Node("bin", op, (x, y), ty),), ty)
        if ty.kind in "iu" and op == "mul":  # -3 * 0 is the integer 0, and 1 / it is +inf: + 0.0 turns the float product's -0.0 into 0.0
            return Node("bin", "add", (Node("bin", op, (x, y), ty), Node("const", 0.0, (), None)), ty)
        return Node("bin", op, (x, y), ty)

    def members(self, node: ast.AST) -> list | None:
        return list(node.elts) if isinstance(node, (ast.List, ast.Tuple)) else None

    def string_leaf(self, node: ast.Compare) -> Node | None:
        if len(node.ops) != 1 or not isinstance(node.left, ast.Name):
            return None
        name = self.backticks.get(node.left.id, node.left.id)
        if name not in self.dtypes or _kind(self.dtypes[name]) in "biufcMm":
            return None
        op, right = node.ops[0], node.comparators[0]
        listed = self.members(right)
        values = listed if listed is not None else [right]
        if not values or not all(isinstance(v, ast.Constant) and isinstance(v.value, str) for v in values):
            raise ValueError(f"column '{name}' is not numeric: it compares with string literals only")
        if isinstance(op, (ast.Eq, ast.In)) and (listed is not None or isinstance(op, ast.Eq)):
            negate = False
        elif isinstance(op, (ast.NotEq, ast.NotIn)) and (listed is not None or isinstance(op, ast.NotEq)):
            negate = True
        else:
            raise ValueError(f"column '{name}' is not numeric: only == != in 'not in' are taken")
        self.host.append(HostLeaf(name, "not in" if negate else "in", tuple(v.value for v in values)))
        return Node("host", len(self.host) - 1, (), BOOL)

    def compare(self, node: ast.Compare) -> Node:
        leaf = self.string_leaf(node)
        if leaf is not None:
            return leaf
        ops, operands = list(node.ops), [node.left, *node.comparators]
        listed = self.members(operands[-1])
        if any(isinstance(op, (ast.In, ast.NotIn)) for op in ops) or listed is not None:
            if len(ops) != 1 or listed is None or not isinstance(ops[0], (ast.In, ast.NotIn, ast.Eq, ast.NotEq)):
                raise ValueError("membership is 'x in [..]', 'x not in [..]', 'x == [..]' or 'x != [..]', and no part of a chain")
            if isinstance(ops[0], (ast.Eq, ast.NotEq)) and not isinstance(operands[0], ast.Name):
                raise ValueError("'== [..]' and '!= [..]' are membership for a plain column only (pandas: lengths must match to compare)")
            x = self.numeric(operands[0], "membership")
            values = []
            for v in listed:
                m = self.visit(v)
                if m.kind != "const" or not math.isfinite(m.value):
                    raise ValueError("the members of a list are finite numeric literals")
                values.append(float(m.value))
            if not values:
                raise ValueError("an empty list")
            return Node("in", (tuple(values), isinstance(ops[0], (ast.NotIn, ast.NotEq))), (x,), BOOL)
        for op in ops:
            if type(op) not in _COMPARE:
                raise ValueError(f"the compare {type(op).__name__} is not taken")
        args = [self.numeric(v, "a compare") for v in operands]
        names = [_COMPARE[type(op)] for op in ops]
        pairs = []
        for k, name in enumerate(names):
            x, y = args[k], args[k + 1]
            if x.kind == "const" and y.kind == "const":
                raise ValueError("a compare of two literals")
            pairs.append((name, *self.rounded(x, y)))
        if len(pairs) == 1:
            return Node("bin", pairs[0][0], pairs[0][1:], BOOL)
        if len(pairs) == 2 and args[1].kind not in ("col", "const"):  # the middle operand is evaluated once
            return Node("chain", (names[0], names[1]), (pairs[0][1], args[1], pairs[1][2]), BOOL)
        out = Node("bin", pairs[0][0], pairs[0][1:], BOOL)
        for name, x, y in pairs[1:]:
            out = Node("bin", "and", (out, Node("bin", name, (x, y), BOOL)), BOOL)
        return out

    @staticmethod
    def rounded(x: Node, y: Node) -> tuple[Node, Node]:
        """A literal against a float32 / float16 operand: numpy compares in that precision."""
        def as_seen(c: Node, other: Node) -> Node:
            if c.kind == "const" and other.ty is not None and other.ty.kind == "f" and other.ty.itemsize < 8:
                with np.errstate(over="ignore"):
                    return Node("const", float(other.ty.type(c.value)), (), None)
            return c

        return as_seen(x, y), as_seen(y, x)


# ---- the compiler -------------------------------------------------------------------------------------------------------------------------
def _need(node: Node) -> int:
    """Sethi-Ullman: the stack slots the node's evaluation needs."""
    if node.kind in ("col", "const", "host"):
        return 1
    if node.kind in ("un", "in"):
        return _need(node.args[0])
    if node.kind == "chain":
        first, middle, last = node.args
        return max(_need(middle), 2 + _need(first), 2 + _need(last))
    a, b = _need(node.args[0]), _need(node.args[1])
    return a + 1 if a == b else max(a, b)


class _Emitter:
    def __init__(self) -> None:
        self.inputs: list[str] = []
        self.code: list[tuple[str, int, int]] = []
        self.consts: list[float] = []
        self.depth = 0
        self.deepest = 0
        self.held: dict[str, int] = {}  # column -> the stack slot that holds its masked value

    def op(self, name: str, arg0: int = 0, arg1: int = 0, grow: int = 0) -> None:
        self.code.append((name, arg0, arg1))
        self.depth += grow
        self.deepest = max(self.deepest, self.depth)

    def input(self, name: str) -> int:
        if name not in self.inputs:
            self.inputs.append(name)
        return self.inputs.index(name)

    def const(self, values: Sequence[float]) -> int:
        """The start of ``values`` in the constant table, found by bit pattern or appended."""
        bits = [np.float64(v).view(np.uint64) for v in values]
        have = [np.float64(v).view(np.uint64) for v in self.consts]
        for start in range(len(have) - len(bits) + 1):
            if have[start:start + len(bits)] == bits:
                return start
        self.consts.extend(float(v) for v in values)
        return len(self.consts) - len(values)

    def emit(self, node: Node) -> None:
        if node.kind == "col":
            if node.value in self.held:
                self.op("dup", self.depth - 1 - self.held[node.value], grow=1)
            else:
                self.op("push_col", self.input(node.value), grow=1)
        elif node.kind == "host":
            self.op("push_col", self.input(f"{HOST_ROW}{node.value}"), grow=1)
        elif node.kind == "const":
            self.op("push_const", self.const([node.value]), grow=1)
        elif node.kind == "un":
            self.emit(node.args[0])
            self.op(node.value)
        elif node.kind == "in":
            members, negate = node.value
            self.emit(node.args[0])
            self.op("in_set", self.const(members), len(members))
            if negate:
                self.op("not")
        elif node.kind == "chain":  # first op1 middle op2 last, the middle evaluated once
            first, middle, last = node.args
            self.emit(middle)
            self.op("dup", 0, grow=1)
            self.emit(first)
            self.op(_FLIPPED[node.value[0]], grow=-1)  # middle flipped(op1) first
            self.op("swap")
            self.emit(last)
            self.op(node.value[1], grow=-1)
            self.op("and", grow=-1)
        else:
            x, y = node.args
            if _need(y) > _need(x):
                self.emit(y)
                self.emit(x)
                if node.value in _FLIPPED:
                    self.op(_FLIPPED[node.value], grow=-1)
                else:
                    if node.value not in _COMMUTATIVE:
                        self.op("swap")
                    self.op(node.value, grow=-1)
            else:
                self.emit(x)
                self.emit(y)
                self.op(node.value, grow=-1)

    def finish(self, results: Sequence[str], keep: bool, host: Sequence[HostLeaf], text: str) -> ExprProgram:
        for what, size, limit in (("EXPR_MAX_STACK", self.deepest, native.EXPR_MAX_STACK), ("EXPR_MAX_INSTR", len(self.code), native.EXPR_MAX_INSTR),
                                  ("EXPR_MAX_CONSTS", len(self.consts), native.EXPR_MAX_CONSTS), ("EXPR_MAX_INPUTS", len(self.inputs), native.EXPR_MAX_INPUTS),
                                  ("EXPR_MAX_RESULTS", len(results), native.EXPR_MAX_RESULTS)):
            if size > limit:
                raise ValueError(f"the expression is too large for one launch: it needs {size}, {what} is {limit}: {text}")
        return ExprProgram(tuple(self.inputs), tuple(self.code), tuple(self.consts), tuple(results), keep, tuple(host), self.deepest)


def parse(text: str, dtypes: Mapping[str, Any], host: list[HostLeaf]) -> Node:
    """The typed tree of a boolean expression; ``host`` collects its string leaves."""
    if not isinstance(text, str) or not text.strip():
        raise ValueError("the expression is empty")
    try:
        source, backticks = rewrite(text)
        tree = ast.parse(source.strip(), mode="eval")
    except SyntaxError as e:
        raise ValueError(f"invalid syntax: {e.msg}") from None
    node = _Typer(dtypes, backticks, host).visit(tree.body)
    if node.ty != BOOL:
        raise ValueError("the expression does not give a boolean per row")
    return node


def compile_query(text: str, dtypes: Mapping[str, Any]) -> ExprProgram:
    """The keep-row program of ``DataFrame.query(text)`` over columns of the dtypes ``dtypes`` (numpy or torch; datetime64 and object say
    what the query cannot use)."""
    host: list[HostLeaf] = []
    e = _Emitter()
    e.emit(parse(text, dtypes, host))
    return e.finish((), True, host, text)


def compile_masks(conditions: Sequence[tuple[str, str]], dtypes: Mapping[str, Any]) -> ExprProgram:
    """``[(column, condition), ...]`` in order: the column is NaN where ``DataFrame.eval(condition)`` holds, and a later condition sees an
    earlier one's masked column — ONE program, the masked columns at the bottom of the stack.  ``SplitNeeded`` where one program cannot
    say it: a column masked twice, or a later condition that reads an earlier INTEGER target (whose dtype, and so numpy's typing of
    the later condition, depends on whether a row was masked)."""
    host: list[HostLeaf] = []
    e = _Emitter()
    for column, text in conditions:
        if column in dtypes and _kind(dtypes[column]) not in "iuf":
            raise ValueError(f"column '{column}' of dtype {dtypes[column]} cannot be masked: a numeric column is needed")
        node = parse(text, dtypes, host)
        if column in e.held:
            raise SplitNeeded(f"column '{column}' is masked twice")
        if any(_kind(dtypes[c]) != "f" and c in _columns_of(node) for c in e.held):
            raise SplitNeeded("a condition reads an integer column that an earlier one masks")
        e.op("push_col", e.input(column), grow=1)
        e.emit(node)
        e.op("nan_where", grow=-1)
        e.held[column] = e.depth - 1
    return e.finish([c for c, _ in conditions], False, host, "; ".join(t for _, t in conditions))


def _columns_of(node: Node) -> set[str]:
    if node.kind == "col":
        return {node.value}
    return set().union(*(_columns_of(a) for a in node.args)) if node.args else set()


def host_leaf(leaf: HostLeaf, column: Any) -> np.ndarray:
    """The string leaf over a host column, as numpy evaluates it: a bool array."""
    a = np.asarray(column, dtype=object).reshape(-1)
    hit = np.zeros(len(a), dtype=bool)
    for v in leaf.values:
        hit |= np.array([isinstance(x, str) and x == v for x in a.tolist()], dtype=bool)
    return ~hit if leaf.op == "not in" else hit
