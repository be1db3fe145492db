"""``apply_column_transformations`` without a GPU: the registry and the constructor's errors (the reference's three cases), the export
and the argument checks of ``atx_obs_column_ops``, the program compiler against a plain numpy interpreter of the specification
(tests/column_ops_restatement.py), the restatement against numpy's own intermediates and the recorded frames
(tests/golden/column_transformations.json), and a record of numpy's own distance from exact arithmetic on the generators the GPU
test uses.

numpy's worst error against exact arithmetic on those generators, this build (printed by the last test; a record of what the
reference does, no bound for the kernel): log 0.500, log1p 0.499, safe_log 0.499, sqrt 0.500, exp 0.605, abs 0, sin 0.510 (0.499
beyond 1e5), sin_deg 0.503, cos 0.561 (0.496 beyond 1e5), cos_deg 0.561 ulps.
"""

from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import column_ops_restatement as R
from anemoi_transform_amd import native, obs
from anemoi_transform_amd.filters import create_filter_by_name, filter_registry
from anemoi_transform_amd.filters.tabular import ApplyColumnTransformations
from anemoi_transform_amd.obs import ColumnOp, IntegerAbs, KernelStep, compile_column_program

CASES = R.load_golden()
BY_ID = {case["id"]: case for case in CASES}
F64, I64 = np.dtype(np.float64), np.dtype(np.int64)


# ---- registration and construction ------------------------------------------------------------------------------------------------------
def test_registered_and_the_reference_constructor_cases():
    """R: tests/tabular_filters/test_apply_column_transformations.py:124-150."""
    assert "apply_column_transformations" in filter_registry.registered
    f = create_filter_by_name("apply_column_transformations", col1={"function": "log"}, lnsp={"function": "safe_log", "source_column": "sp"},
                              s={"function": "sin_deg", "source_column": ["dd"]})
    assert isinstance(f, ApplyColumnTransformations)
    assert f.transformations == [("col1", "col1", "log"), ("lnsp", "sp", "safe_log"), ("s", "dd", "sin_deg")]
    assert repr(f) == "ApplyColumnTransformations(col1=log(col1), lnsp=safe_log(sp), s=sin_deg(dd))"
    with pytest.raises(ValueError):  # :140-145
        create_filter_by_name("apply_column_transformations", col={"function": "unknown_function"})
    with pytest.raises(ValueError):  # :148-150
        create_filter_by_name("apply_column_transformations")
    for bad in ("log", {"source_column": "x"}, None):
        with pytest.raises(ValueError, match="Invalid transformation specification"):
            create_filter_by_name("apply_column_transformations", col=bad)
    with pytest.raises(NotImplementedError, match="2 source columns"):
        create_filter_by_name("apply_column_transformations", col={"function": "log", "source_column": ["a", "b"]})
    with pytest.raises(ValueError, match="Invalid transformation: tan"):  # the function is looked at first, as in the reference
        create_filter_by_name("apply_column_transformations", col={"function": "tan", "source_column": ["a", "b"]})


def test_a_missing_source_column_is_a_key_error_before_any_launch():
    """R: :124-137 — raised by the compiler, on the host, whatever the table holds."""
    pd = pytest.importorskip("pandas")
    f = create_filter_by_name("apply_column_transformations", col1={"function": "log"}, col2={"function": "log1p"})
    for table in (pd.DataFrame({"col1": [0.0, 1.0, 2.0, 3.0, 4.0]}), {"col1": np.arange(5.0)}):
        with pytest.raises(KeyError):
            f(table)
    for column in (np.array([True, False]), np.array(["a", "b"]), np.array([1j, 2j])):
        with pytest.raises(ValueError, match="numeric"):
            create_filter_by_name("apply_column_transformations", x={"function": "abs"})({"x": column})


def test_parity_note_is_said_once_at_construction(caplog):
    import logging

    from anemoi_transform_amd.core import reset_notes

    reset_notes()
    with caplog.at_level(logging.DEBUG, logger="anemoi_transform_amd"):
        create_filter_by_name("apply_column_transformations", x={"function": "log"})
        create_filter_by_name("apply_column_transformations", x={"function": "exp"})
    said = [r for r in caplog.records if "sqrt and abs have numpy's bits" in r.getMessage()]
    assert [r.levelno for r in said] == [logging.WARNING, logging.DEBUG] and "1 ulp" in said[0].getMessage()
    assert not any("read as float64" in r.getMessage() for r in caplog.records)  # said when a narrow column is first met, not here


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_checks_its_arguments():
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "atx.h")).read()
    assert "ATX_API int atx_obs_column_ops(" in header and "apply_column_transformations.py" in header
    assert "atx_obs_column_ops" in native.SIGNATURES
    for name, code in native.COLUMN_OPS.items():  # the codes of the header are the codes of the binding
        assert f"ATX_COLOP_{name.upper()} = {code}" in header
    assert tuple(native.COLUMN_OPS) == R.FUNCTIONS == obs.COLUMN_FUNCTIONS and f"#define ATX_MAX_COLUMN_OPS {native.MAX_COLUMN_OPS}" in header
    lib = native.load()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first

    def call(ops, srcs, ins, outs, n=8, n_ops=None):
        k = len(ops)
        return lib.atx_obs_column_ops(k if n_ops is None else n_ops, (ctypes.c_int32 * k)(*ops), (ctypes.c_int32 * k)(*srcs),
                                      (ctypes.c_void_p * k)(*ins), (ctypes.c_void_p * k)(*outs), n, None)

    assert call([0], [-1], [one], [one], n_ops=0) == native.EINVAL and b"1 .. 16" in lib.atx_last_error()
    assert call([0] * 17, [-1] * 17, [one] * 17, [one] * 17) == native.EINVAL
    assert call([10], [-1], [one], [one]) == native.EINVAL and b"unknown code" in lib.atx_last_error()
    assert call([-1], [-1], [one], [one]) == native.EINVAL
    assert call([0], [0], [one], [one]) == native.EINVAL and b"not an earlier one" in lib.atx_last_error()  # src[0] >= 0
    assert call([0, 4], [-1, 1], [one, None], [None, one]) == native.EINVAL  # itself
    assert call([0, 4], [-1, 2], [one, None], [None, one]) == native.EINVAL  # a later one
    assert call([0], [-1], [None], [one]) == native.EINVAL and b"null column" in lib.atx_last_error()
    assert call([0], [-1], [one], [one], n=-1) == native.EINVAL
    assert lib.atx_obs_column_ops(1, None, None, None, None, 8, None) == native.EINVAL
    assert call([0, 4], [-1, 0], [None, None], [None, None], n=0) == native.OK  # no rows: validated, nothing launched


# ---- the compiler -----------------------------------------------------------------------------------------------------------------------------
def test_compiler_against_the_interpreter_on_random_specifications():
    rng = np.random.default_rng(20261019)
    seen = {"steps": 0, "chained": 0, "dropped": 0, "integer_abs": 0, "split": 0}
    for _ in range(300):
        spec, table = R.random_spec(rng)
        want = R.interpret(spec, table)
        steps = compile_column_program(spec, {name: col.dtype for name, col in table.items()})
        got = R.run_steps(steps, table)
        assert list(got) == list(want)
        for name in want:
            assert R.same_bits(got[name], want[name]), (spec, name)
        kernel = [s for s in steps if isinstance(s, KernelStep)]
        assert sum(len(s.ops) for s in kernel) + sum(isinstance(s, IntegerAbs) for s in steps) == len(spec)
        for a, b in zip(steps, steps[1:]):  # a run is as long as it may be: it ends only when full or at an integer abs
            assert not (isinstance(a, KernelStep) and isinstance(b, KernelStep)) or len(a.ops) == R.MAX_OPS
        seen["steps"] += len(steps)
        seen["chained"] += sum(op.src >= 0 for s in kernel for op in s.ops)
        seen["dropped"] += sum(not op.store for s in kernel for op in s.ops)
        seen["integer_abs"] += sum(isinstance(s, IntegerAbs) for s in steps)
        seen["split"] += sum(len(s.ops) == R.MAX_OPS for s in kernel)
    assert all(count > 20 for count in seen.values()), seen


def _chain(n):
    """x -> t0 -> t1 -> ...: n transformations, each reading the one before."""
    return [(f"t{k}", "x" if k == 0 else f"t{k - 1}", R.FUNCTIONS[k % 10]) for k in range(n)]


def test_sixteen_operations_are_one_run_and_seventeen_are_two():
    steps = compile_column_program(_chain(16), {"x": F64})
    assert len(steps) == 1 and len(steps[0].ops) == 16
    assert [op.src for op in steps[0].ops] == [-1] + list(range(15)) and all(op.store for op in steps[0].ops)
    assert steps[0].ops[3] == ColumnOp("sqrt", "t3", "t2", 2, True)
    steps = compile_column_program(_chain(17), {"x": F64})
    assert [len(s.ops) for s in steps] == [16, 1]
    assert steps[1].ops == (ColumnOp("sin", "t16", "t15", -1, True),)  # across runs a column goes through memory


def test_latest_writer_overwritten_targets_and_repeated_targets():
    spec = [("y", "x", "log"), ("y", "x", "exp"), ("z", "y", "sqrt"), ("x", "x", "abs"), ("w", "x", "sin"), ("y", "y", "cos")]
    (step,) = compile_column_program(spec, {"x": F64})
    assert step.ops == (
        ColumnOp("log", "y", "x", -1, False),  # replaced by the next one: never stored
        ColumnOp("exp", "y", "x", -1, False),  # read by sqrt through a register, replaced by the last one
        ColumnOp("sqrt", "z", "y", 1, True),  # the LATEST earlier writer of y
        ColumnOp("abs", "x", "x", -1, True),  # a float abs stays in the kernel; x itself is read from memory, before this store
        ColumnOp("sin", "w", "x", 3, True),
        ColumnOp("cos", "y", "y", 1, True),
    )
    table = {"x": np.array([0.5, -2.0, np.nan, 4.0])}
    want, got = R.interpret(spec, table), R.run_steps([step], table)
    assert list(got) == list(want) == ["x", "y", "z", "w"] and all(R.same_bits(got[k], want[k]) for k in want)


def test_an_integer_abs_ends_the_run_and_keeps_its_dtype():
    spec = [("a", "x", "log"), ("k", "k", "abs"), ("b", "a", "exp"), ("c", "k", "abs"), ("d", "c", "sqrt"), ("e", "d", "abs"), ("k", "k", "sin"),
            ("f", "k", "abs")]
    steps = compile_column_program(spec, {"x": F64, "k": I64})
    assert steps == [
        KernelStep((ColumnOp("log", "a", "x", -1, True),)),
        IntegerAbs("k", "k"),
        KernelStep((ColumnOp("exp", "b", "a", -1, True),)),  # a was written by an earlier run: through memory
        IntegerAbs("c", "k"),  # the result of an integer abs is an integer column
        KernelStep((ColumnOp("sqrt", "d", "c", -1, True), ColumnOp("abs", "e", "d", 0, True), ColumnOp("sin", "k", "k", -1, True),
                    ColumnOp("abs", "f", "k", 2, True))),  # k is float64 once sin has replaced it: its abs is the kernel's
    ]
    table = {"x": np.array([1.0, 2.0, 3.0]), "k": np.array([-3, 0, 7], dtype=np.int64)}
    want, got = R.interpret(spec, table), R.run_steps(steps, table)
    assert want["c"].dtype == got["c"].dtype == np.int64 and want["f"].dtype == np.float64
    assert all(R.same_bits(got[k], want[k]) for k in want)
    import torch

    assert obs._dtype_kind(torch.int32) == "i" and obs._dtype_kind(torch.uint8) == "u" and obs._dtype_kind(torch.float16) == "f"
    assert obs._dtype_kind(torch.bool) == "b" and obs._dtype_kind(np.dtype("U3")) == "U"
    unsigned = compile_column_program([("a", "u", "abs")], {"u": np.dtype(np.uint16)})
    assert unsigned == [IntegerAbs("a", "u")]
    for name in ("uint8", "uint16", "uint32", "uint64"):
        assert obs._dtype_kind(getattr(torch, name)) == "u" and obs._dtype_kind(np.dtype(name)) == "u"


def test_abs_of_every_integer_dtype_keeps_dtype_and_values():
    """An integer abs runs outside the kernel, so it can be run here: host columns of every width, signed and unsigned (torch has no
    abs for the wider unsigned types; an unsigned column is its own absolute value)."""
    import torch

    for name in ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"):
        info = np.iinfo(name)
        k = np.array([info.min + (1 if info.min < 0 else 0), 0, 3, info.max], dtype=name)
        got = obs.column_ops({"k": k}, [("m", "k", "abs"), ("k", "m", "abs")], dev=torch.device("cpu"))
        for column in got.values():
            assert column.cpu().numpy().dtype == k.dtype and np.array_equal(column.cpu().numpy(), np.abs(k)), name


def test_compiler_errors():
    with pytest.raises(ValueError, match="Invalid transformation: tan"):
        compile_column_program([("a", "x", "tan")], {"x": F64})
    with pytest.raises(KeyError):
        compile_column_program([("a", "x", "log"), ("b", "c", "log")], {"x": F64})
    with pytest.raises(ValueError, match="numeric"):
        compile_column_program([("a", "x", "log")], {"x": np.dtype(bool)})
    assert compile_column_program([], {"x": F64}) == []
    assert compile_column_program([("a", "x", "log"), ("b", "a", "log")], {"x": np.dtype(np.float32)})[0].ops[1].src == 0


# ---- the restatement against numpy and the reference ---------------------------------------------------------------------------------------
def test_arguments_have_numpy_bits():
    """``x + 1e-10`` and ``x * (pi / 180)`` — the kernel's two argument roundings — are numpy's own intermediates, bit for bit."""
    for function in ("safe_log", "sin_deg", "cos_deg"):
        x = R.cases(function)
        with np.errstate(all="ignore"):
            arg = R.argument(function, x)
            if function == "safe_log":
                assert R.same_bits(np.log(arg), R.NUMPY[function](x))
            else:
                assert R.same_bits_or_both_nan(arg, np.deg2rad(x)) and R.same_bits_or_both_nan(arg, np.radians(x))
                assert R.same_bits((np.sin if function == "sin_deg" else np.cos)(arg), R.NUMPY[function](x))
    assert R.RAD == math.pi / 180 == float(np.deg2rad(1.0))


def test_restatement_equals_the_recorded_frames():
    assert [c["id"] for c in CASES][:4] == ["reference_test_apply_column_transformations", "reference_test_add_sine", "reference_test_add_cosine",
                                            "reference_test_safe_log"]
    assert {f"seeded_{f}" for f in R.FUNCTIONS} | {"chained", "int64_abs_and_safe_log"} <= set(BY_ID)
    for case in CASES:
        spec = [(t, s.get("source_column", t) if isinstance(s.get("source_column", t), str) else s["source_column"][0], s["function"])
                for t, s in case["config"].items()]
        got = R.interpret(spec, case["table"])
        assert list(got) == list(case["expected"]), case["id"]  # existing columns in place, new ones appended in config order
        for name, column in case["expected"].items():
            assert R.same_bits(got[name], column), (case["id"], name)  # numpy is numpy: the same build recorded them
        for column, values in case.get("literals", {}).items():
            assert np.allclose(got[column], values)
    ints = BY_ID["int64_abs_and_safe_log"]["expected"]
    assert ints["k"].dtype == ints["k_abs"].dtype == np.int64 and ints["k_log"].dtype == ints["k_sin"].dtype == np.float64
    for function in R.FUNCTIONS:  # every seeded frame holds the specials
        x = BY_ID[f"seeded_{function}"]["table"]["x"]
        assert x.size == 48 and np.isnan(x).any() and np.isinf(x).any() and (x < 0).any() and (np.signbit(x) & (x == 0)).any()


def test_generators_cover_what_the_kernel_can_get_wrong():
    for function in R.FUNCTIONS:
        x = R.cases(function)
        assert x.size == R.N_CASES and np.isnan(x).any() and {np.inf, -np.inf} <= set(x[np.isinf(x)].tolist())
        assert (x < 0).any() and (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
    x = R.cases("log")
    assert ((x > 0) & (x < 2.2250738585072014e-308)).sum() > 50 and (x > 1e300).any() and (np.abs(x - 1.0) < 2e-14).sum() >= 97
    x = R.cases("log1p")
    assert (x == -1.0).any() and ((x > 0) & (x < 1e-300)).any() and (x >= 1e299).any() and x[np.isfinite(x) & (x > -1.5)].max() <= 1e300
    x = R.cases("exp")
    assert (x == -746.0).any() and (x == 710.0).any() and ((x > -745.2) & (x < -708.3)).sum() > 100
    for function in ("sin", "cos"):
        a = np.abs(R.cases(function))
        a = a[np.isfinite(a)]
        assert (a < 2 * math.pi).sum() > 400 and ((a > 1e4) & (a < 1e5)).sum() > 100 and (a >= 1e5).sum() > 100
        near = np.abs(a / (math.pi / 2) - np.round(a / (math.pi / 2)))
        assert ((near < 1e-15) & (a > 1) & (a < 100)).sum() > 100
    for function in ("sin_deg", "cos_deg"):
        x = R.cases(function)
        assert set((np.arange(-8, 9) * 90.0).tolist()) <= set(x.tolist()) and ((x > -720) & (x < 720)).sum() > 900
        assert (np.abs(R.argument(function, x)[np.isfinite(x)]) >= 1e5).sum() > 50
    b = R.budgets("sin_deg", np.array([90.0, 1e5 / R.RAD * 1.01, np.inf]))
    assert b.tolist() == [1.0, 2.0, 2.0] and R.budgets("log", np.zeros(3)).tolist() == [1.0] * 3


def test_numpy_own_error_against_exact_arithmetic_is_recorded():
    """What the reference itself does on the GPU test's generators — a record, not a bound for the kernel: numpy (glibc) stays within
    an ulp of exact arithmetic everywhere, and matches every special value."""
    for function in R.FUNCTIONS:
        x = R.cases(function)
        with np.errstate(all="ignore"):
            err = R.X.ulp_errors(R.NUMPY[function](x), R.exact_cases(function), np.float64)
        far = np.abs(R.argument(function, x)) >= 1e5
        print(f"numpy {function}: {err.max():.3f} ulps" + (f" ({err[far].max():.3f} at arguments beyond 1e5)" if function in ("sin", "cos") else ""))
        assert np.isfinite(err).all() and err.max() <= 1.0, (function, float(err.max()))
