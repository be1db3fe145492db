"""``atx_obs_column_ops`` (csrc/atx_obs_column_ops.hip) on the device, through ``native.obs_column_ops``, ``obs.column_ops`` and the
``apply_column_transformations`` filter, against exact arithmetic (tests/column_ops_restatement.py) and the frames the reference's own
module returned (tests/golden/column_transformations.json).

- Each of the ten functions alone over wave and block edges: ``sqrt`` and ``abs`` have numpy's bits (any NaN for a NaN under ``sqrt``);
  the other eight stay within their budget of the exact function of the argument as numpy rounds it — 1 ulp for log, safe_log, exp
  (the library's own routines) and log1p (the device library's), 1 ulp for sin / cos / sin_deg / cos_deg of an argument below 1e5
  (sincos_moderate) and 2 ulps beyond (the device library's) — and every special value is matched exactly.  No case is left out.
- Fusion changes nothing: a 16-operation program (one launch) and a 17-operation one (two) give the bits of the same operations
  launched one at a time.
- In place, aliasing, ``out = NULL`` and the rows past ``n`` at the C ABI; the caller's tensors are never written.
- The filter on a DataFrame, a dict of arrays and a dict of device tensors: column order, dtypes, residency, the recorded frames.

Measured on an MI355X (profiles/column_ops_ulps.json), worst over the generators, kernel / budget in ulps: log 0.63 / 1, log1p 0.60 / 1,
safe_log 0.71 / 1, exp 0.80 / 1, sin 0.71 / 1 (beyond 1e5: 0.63 / 2), sin_deg 0.71 / 1 (0.69 / 2),
cos 0.70 / 1 (0.55 / 2), cos_deg 0.71 / 1 (0.63 / 2); sqrt and abs: no row unlike numpy.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import column_ops_restatement as R
from anemoi_transform_amd import native, obs
from anemoi_transform_amd.filters import create_filter_by_name

pytestmark = pytest.mark.gpu

GOLDEN = R.load_golden()


def _dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """``torch.equal`` on the bit patterns: a NaN equals the same NaN."""
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _check(function: str, x: np.ndarray, got: np.ndarray, exact=None, label: str = "") -> float:
    """One function's result against numpy's bits (sqrt, abs) or its budget from exact arithmetic; the worst error in ulps."""
    assert got.dtype == np.float64 and got.shape == x.shape
    with np.errstate(all="ignore"):
        want = R.NUMPY[function](x)
    if function == "abs":
        assert R.same_bits(got, want), label
        return 0.0
    if function == "sqrt":
        assert R.same_bits_or_both_nan(got, want), label
        return 0.5
    err = R.X.ulp_errors(got, R.exact(function, x) if exact is None else exact, np.float64)
    over = err > R.budgets(function, x)
    print(f"{function} {label}: {err[np.isfinite(err)].max():.3f} ulps, {int(np.isinf(err).sum())} specials missed")
    assert not over.any(), (function, label, x[over][:5].tolist(), got[over][:5].tolist(), err[over][:5].tolist())
    return float(err.max())


# ---- each function alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ROWS)
@pytest.mark.parametrize("function", R.FUNCTIONS)
def test_each_function_against_exact_arithmetic(function, n):
    rows = R.rows_of(n)
    x = R.cases(function)[rows]
    source = _dev(x)
    got = obs.column_ops({"x": source}, [("y", "x", function)])
    assert list(got) == ["y"] and got["y"].is_cuda and got["y"].shape == (n,) and got["y"].dtype == torch.float64
    _check(function, x, got["y"].cpu().numpy(), R.exact_cases(function)[rows], f"n={n}")
    assert _same(source, _dev(x))


# ---- fusion ---------------------------------------------------------------------------------------------------------------------------------
PROGRAM = [
    ("t0", "a", "safe_log"), ("t1", "t0", "exp"), ("t2", "t1", "sqrt"), ("t3", "t2", "log"),  # depth 4
    ("t4", "b", "sin_deg"), ("t5", "t4", "abs"), ("t6", "t5", "log1p"),  # depth 3
    ("t7", "b", "cos_deg"), ("t8", "t7", "sin"), ("t9", "t8", "cos"),  # depth 3
    ("a", "a", "log1p"),  # a source replaced: what follows reads the new one
    ("t11", "a", "exp"), ("t0", "t3", "abs"),  # t0 written again: the first is never stored
    ("t13", "t0", "sqrt"), ("t14", "b", "cos"), ("t15", "t14", "sin"),
    ("t16", "t11", "log"),  # the seventeenth: a second launch, its operand through memory
]


@pytest.mark.parametrize("n", R.ROWS)
@pytest.mark.parametrize("n_ops,launches", [(16, 1), (17, 2)])
def test_fusion_changes_nothing(monkeypatch, n, n_ops, launches):
    spec = PROGRAM[:n_ops]
    assert {f for _, _, f in spec} == set(R.FUNCTIONS)
    rng = np.random.default_rng(n)
    a = np.resize(np.concatenate([rng.uniform(0.0, 1.0e5, 40), 10.0 ** rng.uniform(-300, 300, 12), R.SPECIALS]), n)
    b = np.resize(np.concatenate([rng.uniform(-720.0, 720.0, 50), np.arange(-4, 5) * 90.0, R.SPECIALS[::-1]]), n)
    table = {"a": _dev(a), "b": _dev(b)}
    calls = []
    real = native.obs_column_ops
    monkeypatch.setattr(native, "obs_column_ops", lambda ops, rows: (calls.append(len(ops)), real(ops, rows))[1])
    fused = obs.column_ops(table, spec)
    assert calls == ([16] if launches == 1 else [16, 1])
    assert list(fused) == list(dict.fromkeys(t for t, _, _ in spec))
    one_by_one = dict(table)
    for op in spec:
        one_by_one.update(obs.column_ops(one_by_one, [op]))
    assert len(calls) == launches + n_ops
    for name, column in fused.items():
        assert _same(column, one_by_one[name]), name
    assert _same(table["a"], _dev(a)) and _same(table["b"], _dev(b))  # the caller's tensors, a replaced one included, are untouched


# ---- in place, aliasing, NULL outputs, the rows past n ----------------------------------------------------------------------------------------
SENTINEL = -12345.678


def _guarded(n: int, values=None) -> tuple[torch.Tensor, torch.Tensor]:
    """``(whole, row)``: a row of n float64 inside an allocation with 32 sentinel elements before and 96 after."""
    whole = torch.full((n + 128,), SENTINEL, dtype=torch.float64, device="cuda")
    row = whole[32:32 + n]
    if values is not None:
        row.copy_(_dev(values))
    return whole, row


def _guards_hold(whole: torch.Tensor, n: int) -> bool:
    return bool((whole[:32] == SENTINEL).all()) and bool((whole[32 + n:] == SENTINEL).all())


@pytest.mark.parametrize("n", R.ROWS)
def test_c_abi_in_place_null_outputs_and_rows_past_n(n):
    code = native.COLUMN_OPS
    x = R.cases("log")[R.rows_of(n)]
    w = R.cases("sin")[R.rows_of(n)]
    # separate outputs: y = log(x), x2 = exp(x), z = sqrt(x2) [register], s = sin(w), w2 = cos(x)
    wx, dx = _guarded(n, x)
    ww, dw = _guarded(n, w)
    outs = [_guarded(n) for _ in range(5)]
    (wy, y), (wx2, x2), (wz, z), (ws, s), (ww2, w2) = outs
    native.obs_column_ops([(code["log"], -1, dx, y), (code["exp"], -1, dx, x2), (code["sqrt"], 1, None, z), (code["sin"], -1, dw, s),
                           (code["cos"], -1, dx, w2)], n)
    assert all(_guards_hold(whole, n) for whole, _ in outs) and _guards_hold(wx, n) and _guards_hold(ww, n)
    assert _same(dx, _dev(x)) and _same(dw, _dev(w))
    # in place: exp writes x after log has read it, cos writes w after sin has read it — a column that a LATER operation writes may be
    # read from memory, and out[t] may be in[t]
    wy_b, y_b = _guarded(n)
    wz_b, z_b = _guarded(n)
    ws_b, s_b = _guarded(n)
    native.obs_column_ops([(code["log"], -1, dx, y_b), (code["exp"], -1, dx, dx), (code["sqrt"], 1, None, z_b), (code["sin"], -1, dw, s_b),
                           (code["cos"], -1, dw, dw)], n)
    assert _same(y_b, y) and _same(dx, x2) and _same(z_b, z) and _same(s_b, s)
    assert _same(dw, obs.column_ops({"w": _dev(w)}, [("c", "w", "cos")])["c"])
    assert all(_guards_hold(whole, n) for whole in (wx, ww, wy_b, wz_b, ws_b))
    # out = NULL: an intermediate that only a later operation takes, and a target that a later operation replaces
    wq, q = _guarded(n)
    native.obs_column_ops([(code["exp"], -1, _dev(x), None), (code["log"], -1, _dev(x), None), (code["sqrt"], 0, None, q)], n)
    assert _same(q, z) and _guards_hold(wq, n)


def test_a_target_equal_to_its_source_leaves_the_callers_tensor_untouched():
    x = R.cases("exp")[R.rows_of(257)]
    source = _dev(x)
    got = obs.column_ops({"x": source}, [("x", "x", "exp"), ("y", "x", "log")])
    assert _same(source, _dev(x)) and got["x"].data_ptr() != source.data_ptr()
    assert _same(got["x"], obs.column_ops({"x": source}, [("e", "x", "exp")])["e"])
    assert _same(got["y"], obs.column_ops({"x": got["x"]}, [("y", "x", "log")])["y"])


def test_bad_arguments_are_refused_by_the_entry_point():
    x = torch.ones(8, dtype=torch.float64, device="cuda")
    y = torch.zeros(8, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="unknown code"):
        native.obs_column_ops([(10, -1, x, y)], 8)
    with pytest.raises(ValueError, match="not an earlier one"):
        native.obs_column_ops([(0, -1, x, None), (4, 1, None, y)], 8)
    with pytest.raises(ValueError, match="1 .. 16"):
        native.obs_column_ops([(0, -1, x, y)] * 17, 8)
    with pytest.raises(ValueError, match="1 .. 16"):
        native.obs_column_ops([], 8)
    assert bool((y == 0).all())  # nothing was launched
    assert obs.column_ops({"x": x}, []) == {}
    empty = obs.column_ops({"x": x[:0]}, [("y", "x", "log")])["y"]
    assert empty.shape == (0,) and empty.dtype == torch.float64
    with pytest.raises(ValueError, match="differ in length"):
        obs.column_ops({"x": x, "z": x[:4]}, [("a", "x", "log"), ("b", "z", "log")])


def test_the_float64_deviation_is_said_when_a_narrow_column_is_first_met(caplog):
    import logging

    from anemoi_transform_amd.core import reset_notes

    reset_notes()
    f = create_filter_by_name("apply_column_transformations", y={"function": "sqrt", "source_column": "x"})
    with caplog.at_level(logging.DEBUG, logger="anemoi_transform_amd"):
        f({"x": np.array([1.0, 4.0])})
        assert not any("read as float64" in r.getMessage() for r in caplog.records)
        out = f({"x": np.array([1.0, 4.0], dtype=np.float32)})
        f({"x": _dev(np.array([1.0, 4.0], dtype=np.float16))})
    said = [r.levelno for r in caplog.records if "read as float64" in r.getMessage()]
    assert said == [logging.INFO, logging.DEBUG] and out["y"].dtype == np.float64 and out["y"].tolist() == [1.0, 2.0]


def test_integer_and_narrow_float_columns():
    k = np.array([-3, 0, 7, np.iinfo(np.int64).min + 1], dtype=np.int64)
    got = obs.column_ops({"k": _dev(k), "h": _dev(np.array([0.5, 2.0, -1.0, np.nan], dtype=np.float32)), "u": _dev(np.array([0, 1, 200, 255], dtype=np.uint8))},
                         [("m", "k", "abs"), ("l", "m", "safe_log"), ("k", "k", "sin"), ("s", "h", "sqrt"), ("v", "u", "abs"), ("e", "v", "exp")])
    assert got["m"].dtype == torch.int64 and got["m"].cpu().numpy().tolist() == np.abs(k).tolist()
    assert got["v"].dtype == torch.uint8 and got["v"].cpu().numpy().tolist() == [0, 1, 200, 255]
    _check("safe_log", np.abs(k).astype(np.float64), got["l"].cpu().numpy(), label="int64 -> float64")
    _check("sin", k.astype(np.float64), got["k"].cpu().numpy(), label="int64 -> float64")
    _check("exp", np.array([0.0, 1.0, 200.0, 255.0]), got["e"].cpu().numpy(), label="uint8 -> float64")
    assert got["s"].dtype == torch.float64  # Deviation: a float32 column is read as float64
    _check("sqrt", np.array([0.5, 2.0, -1.0, np.nan]), got["s"].cpu().numpy())
    for name in ("uint16", "uint32", "uint64"):  # host columns (numpy) and, where torch can hold them, device tensors
        u = np.array([0, 1, 40000, np.iinfo(name).max], dtype=name)
        for column in (u, _dev(u)):
            wide = obs.column_ops({"u": column}, [("v", "u", "abs"), ("r", "v", "sqrt"), ("q", "u", "sqrt")])
            assert wide["v"].is_cuda and wide["v"].cpu().numpy().dtype == u.dtype and np.array_equal(wide["v"].cpu().numpy(), u), name
            _check("sqrt", u.astype(np.float64), wide["r"].cpu().numpy(), label=name)
            assert _same(wide["q"], wide["r"])
    host = obs.column_ops({"k": k}, [("m", "k", "abs"), ("l", "m", "log1p")])  # host columns go up, results are device rows
    assert host["m"].is_cuda and host["m"].dtype == torch.int64 and _same(host["m"], got["m"]) and host["l"].is_cuda


# ---- the filter ---------------------------------------------------------------------------------------------------------------------------------
def _spec_of(config: dict) -> list[tuple[str, str, str]]:
    return [(t, s.get("source_column", t) if isinstance(s.get("source_column", t), str) else s["source_column"][0], s["function"])
            for t, s in config.items()]


def _route(table: dict, route: str):
    if route == "frame":
        import pandas as pd

        return pd.DataFrame(table)
    return {name: (_dev(col) if route == "tensors" else col.copy()) for name, col in table.items()}


def _host(column) -> np.ndarray:
    return column.cpu().numpy() if isinstance(column, torch.Tensor) else np.asarray(column)


@pytest.mark.parametrize("case", GOLDEN, ids=[c["id"] for c in GOLDEN])
def test_filter_one_transformation_at_a_time_against_exact_arithmetic(case):
    """Every transformation of the recorded configuration as a filter of its own, on what the ones before it left: numpy's bits for
    sqrt and abs (an integer abs keeps its dtype), the budget from the exact function of its own operand for the rest; then the whole
    configuration at once gives the same bits."""
    table = {name: col.copy() for name, col in case["table"].items()}
    current = table
    for (target, source, function), (key, entry) in zip(_spec_of(case["config"]), case["config"].items()):
        x = current[source]
        step = create_filter_by_name("apply_column_transformations", **{key: entry})(current)
        assert list(step) == list(current) + ([target] if target not in current else [])
        if function == "abs" and x.dtype.kind in "iu":
            assert step[target].dtype == x.dtype and np.array_equal(step[target], np.abs(x))
        else:
            _check(function, x.astype(np.float64), step[target], label=f"{case['id']}:{target}")
        current = step
    whole = create_filter_by_name("apply_column_transformations", **case["config"])(table)
    assert list(whole) == list(current) == list(case["expected"])
    for name in whole:
        assert R.same_bits(whole[name], current[name]), name


_ARRAYS: dict = {}


def _arrays_route(case) -> dict:
    """The whole configuration on a dict of arrays, once per case: what the other routes are compared with bit for bit."""
    if case["id"] not in _ARRAYS:
        _ARRAYS[case["id"]] = create_filter_by_name("apply_column_transformations", **case["config"])(_route(case["table"], "arrays"))
    return _ARRAYS[case["id"]]


@pytest.mark.parametrize("route", ["frame", "arrays", "tensors"])
@pytest.mark.parametrize("case", GOLDEN, ids=[c["id"] for c in GOLDEN])
def test_filter_routes_against_the_recorded_frames(case, route):
    """Every route gives, bit for bit, what the dict-of-arrays route gives — which
    test_filter_one_transformation_at_a_time_against_exact_arithmetic holds to numpy's bits (sqrt, abs) and to the budgets (the rest)
    — so a value that lost digits on its way into or out of a DataFrame or a tensor fails here.  Against the recorded frames: equal
    bits for untouched columns and for columns that only sqrt / abs made.  np.allclose is kept for the reference's own literals alone."""
    table = _route(case["table"], route)
    before = table.copy() if route == "frame" else {k: (v.clone() if route == "tensors" else v.copy()) for k, v in table.items()}
    result = create_filter_by_name("apply_column_transformations", **case["config"])(table)
    # the kind of table that went in, never the caller's object, which is untouched
    assert result is not table and type(result) is type(table)
    if route == "frame":
        assert table.equals(before)
    else:
        assert all(_same(table[k], before[k]) if route == "tensors" else R.same_bits(table[k], before[k]) for k in before)
    names = list(result.columns) if route == "frame" else list(result)
    assert names == list(case["expected"])  # existing columns keep their positions, new ones follow in config order
    targets = dict.fromkeys(case["config"])
    spec = _spec_of(case["config"])
    only_bit_equal = {}  # a column whose whole history is sqrt / abs of table columns has numpy's bits
    for target, source, function in spec:
        only_bit_equal[target] = function in R.BIT_EQUAL and only_bit_equal.get(source, source in case["table"])
    held = _arrays_route(case)  # held to the budgets, transformation by transformation, by the test above
    for name, want in case["expected"].items():
        column = result[name]
        if route == "tensors":
            assert isinstance(column, torch.Tensor) and column.is_cuda, name  # residency: new columns and old ones stay in HBM
        elif route == "arrays":
            assert isinstance(column, np.ndarray), name
        got = _host(column.to_numpy() if route == "frame" else column)
        assert got.dtype == want.dtype, (name, got.dtype, want.dtype)  # float64, and an int64 abs stays int64
        assert R.same_bits(got, held[name]), (route, name)  # every route gives the bits of the arrays route
        if name not in targets:
            assert R.same_bits(got, want), name
        elif want.dtype.kind in "iu":
            assert np.array_equal(got, want), name
        elif only_bit_equal[name]:
            assert R.same_bits_or_both_nan(got, want), name
    for name, values in case.get("literals", {}).items():  # R: tests/tabular_filters/test_apply_column_transformations.py:73-74, :97-98
        assert np.allclose(_host(result[name].to_numpy() if route == "frame" else result[name]), values)
    for name, function in case.get("numpy", {}).items():  # R: :46-50, :120-121
        source = case["config"][name].get("source_column", name)
        with np.errstate(all="ignore"):
            assert np.allclose(_host(result[name].to_numpy() if route == "frame" else result[name]), R.NUMPY[function](case["table"][source]),
                               equal_nan=True)
