"""``atx_pressure_at_height_stack`` (csrc/atx_vertical.hip) held in ulps against the exact column statement of tests/exact_statements.py.

The kernel's contract is float64 arithmetic for both widths, statement by statement in numpy's order, one rounding at the store:

- float32: every finite result within 0.5 + C64 2^-29 float32 ulps of exact (C64 float64 ulps are C64 2^-29 float32 ulps) — derived, not
  measured; it is < 0.501 for every C64 below.
- float64: per case and height class the kernel's worst <= 2 x numpy's worst on the same columns + SLACK, under the ceiling C64.  2 x:
  kernel and numpy evaluate the same statements in the same order with IEEE operations and no contraction; the one primitive that
  differs is the logarithm — atx_log is budgeted at 1 ulp, glibc's is at about half that — and near the ground its error enters alpha
  amplified ~1000 x, so the kernel may carry up to twice numpy's share of it.
- special values (NaN, +-inf) exactly where the restatement has them; the five storage shapes byte-identical to each other; nothing
  written beyond out[:n_pts]; the inputs untouched.

The checks are plain functions of (statement, results), so tests/test_column_checks_catch_defects.py can run them on the CPU against
deliberately wrong restatements: every assertion here has been seen to fail for the defect it is there for.
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import exact_statements as X
import vertical_restatement as vr
from anemoi_transform_amd import native
from anemoi_transform_amd.stack import COLUMNS, FIELDS
from test_exact_statements import NUMPY_WORST_COLUMN
from test_gpu_ulp_budgets import SLACK

pytestmark = pytest.mark.gpu

SHAPES = ("columns", "columns-pitch+1", "columns-base+1", "fields", "fields-pitch+3")
CANARY = 7.25


def c64(n_lev: int, group: str, cls: str) -> int:
    """The float64 ceiling (ulps) of a height class: 2 x numpy's PINNED worst (tests/test_exact_statements.py::NUMPY_WORST_COLUMN,
    measured on the CPU with the exact evaluator) + SLACK, rounded up to the next integer."""
    return math.ceil(2.0 * NUMPY_WORST_COLUMN[(n_lev, group, cls)][0] + SLACK)


# The ceilings written out (float64 ulps; the derivation is c64 above, and test_ceilings_are_derived holds the two together).
# (n_lev, group): (near ground, 100 m, aloft, above top)
C64 = {
    (1, X.PHYSICAL): (3, 3, 6, 2), (1, X.ODD): (3, 4, 5, 2),
    (2, X.PHYSICAL): (491, 6, 6, 9), (2, X.ODD): (416, 108, 155, 225),
    (3, X.PHYSICAL): (3, 4, 159, 21), (3, X.ODD): (113, 89, 83, 25),
    (60, X.PHYSICAL): (4, 19, 193, 77), (60, X.ODD): (350, 293, 300, 104),
    (137, X.PHYSICAL): (10, 134, 970, 194), (137, X.ODD): (408, 444, 794, 159),
}


def ceiling(n_lev, case, cls) -> int:
    return C64[(n_lev, X.CASE_GROUP[case])][X.HEIGHT_CLASSES.index(cls)]


def f32_bound(n_lev, case, cls) -> float:
    return 0.5 + ceiling(n_lev, case, cls) * 2.0**-29


# ---- storage ---------------------------------------------------------------------------------------------------------------------
def store(values: np.ndarray, shape: str, dev) -> tuple[torch.Tensor, int, int]:
    """``[n_lev, n_pts]`` values in one of the five storage shapes, every padding element NaN: (stack tensor, pitch, layout).
    "pitch+1" means a pitch that is NOT a multiple of the 16-byte vector (n_lev + 1, or n_lev + 2 where n_lev + 1 is one);
    "base+1" keeps the aligned pitch and starts the stack one element into a larger allocation."""
    n_lev, n_pts = values.shape
    layout = COLUMNS if shape.startswith("columns") else FIELDS
    rows, row_len = (n_pts, n_lev) if layout == COLUMNS else (n_lev, n_pts)
    per16 = 16 // values.itemsize
    pitch = -(-row_len // per16) * per16
    if shape == "columns-pitch+1":
        pitch = row_len + 1 if (row_len + 1) % per16 else row_len + 2
    if shape == "fields-pitch+3":
        pitch = row_len + 3
    dtype = torch.float32 if values.dtype == np.float32 else torch.float64
    off = 1 if shape == "columns-base+1" else 0
    flat = torch.full((rows * pitch + per16 + off,), float("nan"), dtype=dtype, device=dev)
    data = flat[off: off + rows * pitch].view(rows, pitch)
    data[:, :row_len] = torch.from_numpy(np.ascontiguousarray(values.T if layout == COLUMNS else values)).to(dev)
    if str(dev) != "cpu":
        assert (data.data_ptr() % 16 != 0) == (off == 1)
    return data, pitch, layout


def run_case(kernel, dev, t, q, sp, A, B, heights, shape, n_pts=None) -> np.ndarray:
    """The kernel on the first ``n_pts`` columns (cyclically repeated beyond the case's own) at every height: ``[n_heights, n_pts]``.
    Asserts what every call must leave alone: the canary beyond out[:n_pts], and t, q, sp byte for byte."""
    n_lev, m = t.shape
    n_pts = m if n_pts is None else n_pts
    cols = np.arange(n_pts) % m
    t, q, sp = np.ascontiguousarray(t[:, cols]), np.ascontiguousarray(q[:, cols]), np.ascontiguousarray(sp[cols])
    (ts, pitch, layout), (qs, _, _) = store(t, shape, dev), store(q, shape, dev)
    spd = torch.from_numpy(sp).to(dev)
    Ad, Bd = torch.from_numpy(np.asarray(A, np.float64)).to(dev), torch.from_numpy(np.asarray(B, np.float64)).to(dev)
    before = [x.clone() for x in (ts, qs, spd)]
    bits = torch.int32 if ts.dtype == torch.float32 else torch.int64
    got = []
    for h in heights:
        out = torch.full((n_pts + 67,), CANARY, dtype=ts.dtype, device=dev)
        kernel(ts, qs, spd, Ad, Bd, out, n_pts=n_pts, n_lev=n_lev, pitch=pitch, layout=layout, height=h)
        assert (out[n_pts:] == CANARY).all(), f"{shape}, height {h}: written beyond out[:n_pts]"
        got.append(out[:n_pts].cpu().numpy())
    for x, b in zip((ts, qs, spd), before):
        assert torch.equal(x.view(bits), b.view(bits)), f"{shape}: an input stack was modified"
    return np.stack(got)


# ---- the checks (plain functions: the CPU stand-in test drives them too) ---------------------------------------------------------------
def check_specials(got: np.ndarray, want64: np.ndarray, what: str) -> None:
    """NaN positions and infinities exactly as the restatement's (rounded to the kernel's dtype)."""
    with np.errstate(all="ignore"):
        want = want64.astype(got.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ from the restatement's at {np.argwhere(np.isnan(got) != np.isnan(want))[:5].tolist()}"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), f"{what}: infinities differ from the restatement's"


def check_ulps(st: X.ColumnStatement, case: str, got: np.ndarray, report=None) -> None:
    """``got[n_heights, n_pts]`` of one case (columns repeating cyclically) against the exact statement: specials, then per height class
    the float32 or float64 rule of the module docstring."""
    f32 = st.dtype == np.float32
    assert got.dtype == st.dtype
    m = st.numpy_out[case].shape[1]
    cols = np.arange(got.shape[1]) % m
    check_specials(got, st.numpy_out[case][:, cols], f"n_lev {st.n_lev} {case}")
    for cls in X.HEIGHT_CLASSES:
        worst, ref = 0.0, 0.0
        for j, (h, c) in enumerate(st.heights):
            if c != cls:
                continue
            err = st.errors(case, j, got[j])
            assert not np.isinf(err).any(), f"n_lev {st.n_lev} {case}, height {h}: a special value against a finite exact one, column {int(np.argmax(err))}"
            worst = max(worst, float(err.max()))
            e = st.numpy_errors(case, j)[np.unique(cols)]
            ref = max(ref, float(e[np.isfinite(e)].max(initial=0.0)))
        bound = f32_bound(st.n_lev, case, cls) if f32 else min(2.0 * ref + SLACK, ceiling(st.n_lev, case, cls))
        if report is not None:
            key = (st.n_lev, np.dtype(st.dtype).name, X.CASE_GROUP[case], cls)
            k, n, b = report.get(key, (0.0, 0.0, 0.0))
            report[key] = (max(k, worst), max(n, ref), f32_bound(st.n_lev, case, cls) if f32 else ceiling(st.n_lev, case, cls))
        assert worst <= bound, f"n_lev {st.n_lev} {np.dtype(st.dtype).name} {case}, {cls}: kernel {worst:.4f} ulps > {bound:.4f} (numpy {ref:.4f})"


def check_routes_agree(results: dict, what: str) -> None:
    """{shape: got}: byte-identical results whatever the storage — the arithmetic of a column does not depend on how it was loaded."""
    shapes = list(results)
    bits = np.int32 if results[shapes[0]].dtype == np.float32 else np.int64
    for s in shapes[1:]:
        same = results[s].view(bits) == results[shapes[0]].view(bits)
        assert same.all(), f"{what}: {s} differs from {shapes[0]} at (height, column) {np.argwhere(~same)[:5].tolist()}"


# ---- the tests -------------------------------------------------------------------------------------------------------------------
REPORT: dict = {}
_RESULTS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        print("\ncolumn kernel, max ulps against the exact statement (kernel / numpy's own / ceiling):")
        for (n, dt, group, cls), (k, ref, bound) in sorted(REPORT.items()):
            print(f"  n_lev {n:<4} {dt:<8} {group:<17} {cls:<12} kernel {k:9.4f}   numpy {ref:9.4f}   bound {bound:.6g}")


def results(dev, dtype, n_lev, shape) -> dict:
    key = (np.dtype(dtype).name, n_lev, shape)
    if key not in _RESULTS:
        st = X.column_statement(dtype, n_lev)
        hs = [h for h, _ in st.heights]
        _RESULTS[key] = {case: run_case(native.pressure_at_height_stack, dev, t, q, sp, st.A, st.B, hs, shape)
                         for case, (t, q, sp) in st.cases.items()}
    return _RESULTS[key]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n_lev", X.COLUMN_N_LEV)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_column_kernel_against_exact(dev, dtype, n_lev, shape):
    st = X.column_statement(dtype, n_lev)
    for case, got in results(dev, dtype, n_lev, shape).items():
        check_ulps(st, case, got, REPORT)


@pytest.mark.parametrize("n_lev", X.COLUMN_N_LEV)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_storage_routes_agree_bit_for_bit(dev, dtype, n_lev):
    """columns (16-byte loads), columns-pitch+1 and columns-base+1 (the scalar-load instantiation and its second walk), fields and
    fields-pitch+3: the same bytes."""
    st = X.column_statement(dtype, n_lev)
    per_shape = {shape: results(dev, dtype, n_lev, shape) for shape in SHAPES}
    for case in st.cases:
        check_routes_agree({shape: per_shape[shape][case] for shape in SHAPES}, f"n_lev {n_lev} {case}")


@pytest.mark.parametrize("shape", ["columns", "columns-pitch+1", "fields"])
@pytest.mark.parametrize("n_lev", [3, 137])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_workgroup_edges(dev, dtype, n_lev, shape):
    """n_pts at the edges of the 64-lane wave and the 256-lane workgroup, on the first columns of the atmosphere and bent cases."""
    st = X.column_statement(dtype, n_lev)
    hs = [h for h, _ in st.heights]
    for n_pts in (1, 63, 64, 255, 256, 257, 1000):
        for case in ("atmosphere", "bent"):
            t, q, sp = st.cases[case]
            check_ulps(st, case, run_case(native.pressure_at_height_stack, dev, t, q, sp, st.A, st.B, hs, shape, n_pts=n_pts))


def _raw(dev, **change):
    """atx_pressure_at_height_stack through native._call on a valid 10 x 4 float64 column stack, with arguments replaced."""
    x = torch.full((10, 4), 250.0, dtype=torch.float64, device=dev)
    sp = torch.full((10,), 1.0e5, dtype=torch.float64, device=dev)
    A, B = (torch.from_numpy(c).to(dev) for c in X.hybrid_column(4))
    out = torch.zeros(10, dtype=torch.float64, device=dev)
    a = dict(t=x.data_ptr(), q=x.data_ptr(), sp=sp.data_ptr(), A=A.data_ptr(), B=B.data_ptr(), n_pts=10, n_lev=4, pitch=4, dtype=native.F64,
             layout=native.COLUMNS, height=2.0, out=out.data_ptr())
    a.update(change)
    native._call("atx_pressure_at_height_stack", a["t"], a["q"], a["sp"], a["A"], a["B"], a["n_pts"], a["n_lev"], a["pitch"], a["dtype"],
                 a["layout"], a["height"], a["out"], native._stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_kernel_rejects_bad_arguments(dev):
    """The argument checks of atx_pressure_at_height_stack, through native._call's exception mapping.  None of these launches."""
    assert np.isfinite(_raw(dev)).all() and (_raw(dev) != 0).all()  # the valid call
    with pytest.raises(ValueError, match="bad dtype 9"):  # ATX_EINVAL
        _raw(dev, dtype=9)
    with pytest.raises(ValueError, match="bad layout 5"):
        _raw(dev, layout=5)
    with pytest.raises(ValueError, match="bad sizes"):
        _raw(dev, n_lev=0)
    with pytest.raises(ValueError, match="bad sizes"):
        _raw(dev, n_pts=-1)
    with pytest.raises(AssertionError, match="pitch 3 too small"):  # ATX_ESHAPE: COLUMNS wants pitch >= n_lev
        _raw(dev, pitch=3)
    with pytest.raises(AssertionError, match="pitch 9 too small"):  # FIELDS wants pitch >= n_pts
        _raw(dev, layout=native.FIELDS, pitch=9)
    for name in ("A", "B"):
        with pytest.raises(ValueError, match="null A / B"):
            _raw(dev, **{name: None})
    for name in ("t", "q", "sp", "out"):
        with pytest.raises(ValueError, match="null pointer"):
            _raw(dev, **{name: None})
    # an empty stack may have no storage: ATX_OK, nothing launched, nothing written
    assert (_raw(dev, n_pts=0, t=None, q=None, sp=None, out=None) == 0).all()
