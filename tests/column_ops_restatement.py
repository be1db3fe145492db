"""``apply_column_transformations`` stated in numpy, independent of the package, with what its tests share: the interpreter of a list
of transformations (a loop of numpy calls over a dict — the reference's statement), an evaluator of the compiled steps that honours
``src`` and ``store``, seeded random specifications, the input generators of the ten functions, their exact values (mpmath, through
tests/exact_statements.py) and budgets, and the golden file.

The statement: ``table[target] = f(table[source])`` for every transformation in order, ``f`` one of ten numpy expressions.  Against
exact arithmetic every function is measured on the ARGUMENT AS NUMPY ROUNDS IT — ``x + 1e-10`` for ``safe_log``, ``x * (pi / 180)`` for
``sin_deg`` / ``cos_deg`` (``np.deg2rad``'s product; tests/test_column_ops_host.py holds both bit for bit against numpy) — so the error
of that one rounding, which numpy's result carries as well, is not charged to the function.
"""

from __future__ import annotations

import json
import math
import os

import mpmath
import numpy as np

import exact_statements as X

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "column_transformations.json")
ROWS = (1, 63, 64, 65, 257, 4099)  # wave and block edges, a partial last block, more than one block
MAX_OPS = 16
RAD = math.pi / 180.0

# R: filters/tabular/apply_column_transformations.py:18-42, in its order
NUMPY = {
    "log": np.log,
    "log1p": np.log1p,
    "safe_log": lambda x: np.log(x + 1e-10),
    "sqrt": np.sqrt,
    "exp": np.exp,
    "abs": np.abs,
    "sin": np.sin,
    "sin_deg": lambda x: np.sin(np.deg2rad(x)),
    "cos": np.cos,
    "cos_deg": lambda x: np.cos(np.deg2rad(x)),
}
FUNCTIONS = tuple(NUMPY)
BIT_EQUAL = ("sqrt", "abs")  # numpy's bits; the other eight are held in ulps


# ---- the statement ------------------------------------------------------------------------------------------------------------------
def interpret(spec, table: dict) -> dict:
    """The reference's loop: every transformation in order over a copy of the table."""
    table = dict(table)
    with np.errstate(all="ignore"):
        for target, source, function in spec:
            table[target] = NUMPY[function](table[source])
    return table


def run_steps(steps, table: dict) -> dict:
    """The compiled steps (``obs.compile_column_program``) evaluated with numpy as the launches evaluate them: an operation with
    ``src >= 0`` takes the result of that operation of its step, one with ``src < 0`` reads the table AS IT WAS BEFORE THE STEP (every
    output of a launch is a fresh row), a result with ``store`` False is written nowhere."""
    table = dict(table)
    with np.errstate(all="ignore"):
        for step in steps:
            if not hasattr(step, "ops"):  # IntegerAbs
                assert table[step.source].dtype.kind in "iu"
                table[step.target] = np.abs(table[step.source])
                continue
            assert 1 <= len(step.ops) <= MAX_OPS
            results, written = [], {}
            for t, op in enumerate(step.ops):
                assert -1 <= op.src < t
                if op.src >= 0:
                    assert step.ops[op.src].target == op.source
                    x = results[op.src]
                else:
                    assert op.source not in [earlier.target for earlier in step.ops[:t]], "a column an earlier operation writes is read from memory"
                    x = np.asarray(table[op.source], dtype=np.float64)
                results.append(NUMPY[op.function](x))
                if op.store:
                    assert op.target not in written
                    written[op.target] = results[-1]
                else:
                    assert any(later.target == op.target for later in step.ops[t + 1:])
            table.update({target: written[target] for target in dict.fromkeys(op.target for op in step.ops)})  # new columns in spec order
    return table


def random_spec(rng, n_rows: int = 7):
    """``(spec, table)``: 1 .. 40 transformations over 1 .. 6 float64 / int64 columns — sources repeat, targets are reused as sources and
    overwritten, new columns appear."""
    n_cols = int(rng.integers(1, 7))
    table = {}
    for c in range(n_cols):
        if rng.random() < 0.3:
            table[f"c{c}"] = rng.integers(-5, 6, n_rows).astype(np.int64)
        else:
            col = rng.normal(0.0, 3.0, n_rows)
            col[rng.integers(n_rows)] = rng.choice([np.nan, np.inf, -np.inf, 0.0, -0.0])
            table[f"c{c}"] = col
    names = list(table)
    spec = []
    for _ in range(int(rng.integers(1, 41))):
        source = names[int(rng.integers(len(names)))]
        target = names[int(rng.integers(len(names)))] if rng.random() < 0.7 else f"new{int(rng.integers(4))}"
        spec.append((target, source, FUNCTIONS[int(rng.integers(len(FUNCTIONS)))]))
        if target not in names:
            names.append(target)
    return spec, table


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(a.view(np.int64), b.view(np.int64)) if a.dtype == np.float64 else np.array_equal(a, b)


def same_bits_or_both_nan(a, b) -> bool:
    """Bit for bit, a NaN counted as equal to any NaN (numpy's sqrt of a negative number has the sign bit set, the device's has not)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(both | (a.view(np.int64) == b.view(np.int64))))


# ---- arguments, exact values, budgets -------------------------------------------------------------------------------------------------
def argument(function: str, x: np.ndarray) -> np.ndarray:
    """What numpy hands to log / sin / cos: the one rounding that belongs to the statement, not to the function."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        if function == "safe_log":
            return x + 1e-10
        if function in ("sin_deg", "cos_deg"):
            return x * RAD
    return x


def log1p_exact(x: float):
    if math.isnan(x) or x < -1:
        return math.nan
    if x == -1:
        return -math.inf
    if math.isinf(x) or x == 0:
        return x  # +inf; log1p(+-0) = +-0
    return mpmath.log1p(x)


def sqrt_exact(x: float):
    if math.isnan(x) or x < 0:
        return math.nan
    if x == 0 or math.isinf(x):
        return x
    return mpmath.sqrt(x)


_EXACT_FN = {"log": X.log_exact, "safe_log": X.log_exact, "log1p": log1p_exact, "sqrt": sqrt_exact, "exp": X.exp_exact,
             "abs": lambda x: abs(x), "sin": X.sin_exact, "sin_deg": X.sin_exact, "cos": X.cos_exact, "cos_deg": X.cos_exact}


def exact(function: str, x: np.ndarray) -> np.ndarray:
    """The exact function of ``argument(function, x)``: an object array of mpf, or Python floats where the value is special."""
    return X.exact_values(_EXACT_FN[function], argument(function, x))


def budgets(function: str, x: np.ndarray) -> np.ndarray:
    """Per element, ulps from the exact value, from the code (csrc/atx_common.hpp, the HIP math tables): atx_log and atx_exp <= 1, the
    device library's log1p 1; sincos_moderate < 1 for |argument| < 1e5, the device library's sincos 2 beyond; sqrt correctly rounded
    and abs exact: 0.5 and 0 — they are held to numpy's bits instead."""
    if function in ("sin", "sin_deg", "cos", "cos_deg"):
        return np.where(np.abs(argument(function, x)) < 1.0e5, 1.0, 2.0)
    return np.full(np.asarray(x).shape, {"sqrt": 0.5, "abs": 0.0}.get(function, 1.0))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -2.5, -1e300, -5e-324, 5e-324, 1.0, 2.2250738585072014e-308])
N_CASES = 2048


def cases(function: str) -> np.ndarray:
    """``N_CASES`` float64 inputs of one function: its ranges, its edges, and +-0, +-inf, NaN and negative values for every one."""
    rng = np.random.default_rng(1000 + FUNCTIONS.index(function))
    positive = [2.0 ** rng.uniform(-1074.0, 1023.99, 600),  # the whole exponent range, subnormals included
                rng.uniform(5e-324, 2.2250738585072014e-308, 100), rng.uniform(3.0e4, 1.1e5, 200), X.ladder(1.0, np.float64, 48)]
    if function in ("log", "safe_log", "sqrt"):
        parts = positive + [10.0 ** rng.uniform(-12.0, -8.0, 100), rng.uniform(0.0, 10.0, 300)]  # around safe_log's 1e-10
    elif function == "log1p":
        parts = [rng.uniform(-1.0, 1.0, 400), 10.0 ** rng.uniform(-1.0, 300.0, 400), 10.0 ** rng.uniform(-320.0, -1.0, 300),
                 -(10.0 ** rng.uniform(-320.0, -1.0, 300)), np.nextafter(-1.0, 0.0) + np.arange(48) * 2.0 ** -53, [-1.0, 1e300],
                 X.ladder(0.41421356237309515, np.float64, 24), -X.ladder(0.2928932188134524, np.float64, 24)]
    elif function == "exp":
        parts = [rng.uniform(-746.0, 710.0, 800), rng.uniform(9.0, 12.0, 200), X.ladder(709.782712893384, np.float64, 48),
                 rng.uniform(-745.2, -708.3, 200), rng.uniform(-1e-3, 1e-3, 200), 10.0 ** rng.uniform(-300.0, -8.0, 100), [-746.0, 710.0, 1e30, -1e30]]
    elif function == "abs":
        parts = positive + [-p for p in positive] + [np.array([-0x0007FFFFFFFFEDCC], dtype=np.int64).view(np.float64)]  # a NaN with the sign set and a payload
    elif function in ("sin", "cos"):
        near = X.near_multiples(math.pi / 2, 60, np.float64, rng, steps=2)
        parts = [rng.uniform(-2 * math.pi, 2 * math.pi, 500), rng.uniform(-1.0e5, 1.0e5, 400), near,
                 10.0 ** rng.uniform(5.0, 300.0, 150), -(10.0 ** rng.uniform(5.0, 8.0, 50)), 10.0 ** rng.uniform(-300.0, -3.0, 100),
                 -(10.0 ** rng.uniform(-30.0, -3.0, 50)), np.nextafter(1.0e5, [0.0, np.inf])]
    else:  # sin_deg, cos_deg
        parts = [rng.uniform(-720.0, 720.0, 900), np.arange(-8, 9) * 90.0, X.near_multiples(90.0, 8, np.float64, rng, steps=4),
                 rng.uniform(-1.0e5 / RAD, 1.0e5 / RAD, 200), 10.0 ** rng.uniform(7.0, 300.0, 100), 10.0 ** rng.uniform(-300.0, -5.0, 100)]
    x = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in parts] + [SPECIALS])
    assert x.size <= N_CASES, (function, x.size)
    return np.concatenate([x, np.resize(x, N_CASES - x.size)])


_CACHE: dict = {}


def exact_cases(function: str) -> np.ndarray:
    """``exact(function, cases(function))``, computed once per process."""
    if function not in _CACHE:
        _CACHE[function] = exact(function, cases(function))
    return _CACHE[function]


def rows_of(n: int) -> np.ndarray:
    """The generator's cases the n rows of a launch hold (cyclically beyond ``N_CASES``)."""
    return np.arange(n) % N_CASES


# ---- the golden file ------------------------------------------------------------------------------------------------------------------
def encode(a) -> dict:
    """An array as its dtype and integer bit patterns: equality of what comes back is exact, NaN payloads and -0.0 included."""
    a = np.ascontiguousarray(a)
    bits = a.view(np.int64) if a.dtype == np.float64 else a
    return {"dtype": a.dtype.name, "bits": bits.reshape(-1).tolist()}


def decode(spec: dict) -> np.ndarray:
    dtype = np.dtype(spec["dtype"])
    return np.array(spec["bits"], dtype=np.int64 if dtype == np.float64 else dtype).view(dtype)


def load_golden() -> list[dict]:
    """The recorded cases: ``id``, ``config``, ``table`` and ``expected`` (name -> column, in column order), ``literals`` where the
    reference's test states them."""
    with open(GOLDEN) as f:
        found = json.load(f)["cases"]
    for case in found:
        for key in ("table", "expected"):
            case[key] = {name: decode(spec) for name, spec in case[key].items()}
    return found
