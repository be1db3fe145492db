"""The combine operators and ATX_OP_EXP / ATX_OP_LOG held in ulps against exact (128-bit) arithmetic (tests/exact_statements.py).

- Single-function operators: max ulps from the exact function of the argument as the statement rounds it <= a budget derived from the
  code (below, per route of the library's knobs).
- Composed statements (humidity, wind direction): the kernel's worst error, per input case, within SLACK ulps of numpy's own worst on
  the same inputs, and under an absolute ceiling per operator.
- Special values (NaN, +-inf, signed zeros) as the statement gives them; the pure-arithmetic operators bit for bit.

Every operator runs in both dtypes, both layouts, and once with a pitch that is not a multiple of the 16-byte vector.  A library built
with other knobs (tools/build_variant.sh, loaded through ATX_LIBRARY) is measured against the budgets of ITS routes when
ATX_LIBRARY_DEFINES names the defines it was built with (e.g. ``ATX_LIBRARY_DEFINES="-DATX_FAST_EXP=0"``).
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import exact_statements as X
from ulp_budgets import FAST_SINCOS, LIB64, budgets  # the tables and their derivation: tests/ulp_budgets.py
from anemoi_transform_amd import native
from anemoi_transform_amd.stack import COLUMNS, FIELDS
from oracle import oracle

pytestmark = pytest.mark.gpu

SLACK = 2.0  # composed statements: ulps the kernel may lose beyond numpy's own worst error on the same case


# composed statements: an absolute ceiling per operator (ulps; the direction of xy_to_polar in ulps of 360 degrees), above numpy's own
# worst (tests/test_exact_statements.py pins it) by a margin, far below what a lost refinement step costs (2^-46 relative: ~100 ulps f64)
CEILING = {"atan2_deg": 4.0, "xy_to_polar": 4.0, "r_to_d": 6.0, "d_to_r": 90.0, "q_to_r": 48.0, "r_to_q": 48.0, "q_to_r_level": 48.0,
           "r_to_q_level": 48.0,
           # the two dewpoint forms of q_height.py: ceil(1.1 x + 0.1 + SLACK) of numpy's pinned worst x over both dtypes (the top of
           # the window it is pinned in, plus the slack) — q_to_d: numpy 1.89 (float64) / 1.99 (float32) -> 5; d_to_q: numpy 23.69 /
           # 39.15 -> 46
           "q_to_d": 5.0, "d_to_q": 46.0}

COMB = {  # statement -> (operator, flags, outputs)
    "cos_sin": (native.COMB_COS_SIN, 0, 2),
    "cos_sin_deg": (native.COMB_COS_SIN, native.COMB_DEGREES, 2),
    "atan2": (native.COMB_ATAN2, 0, 1),
    "atan2_deg": (native.COMB_ATAN2, native.COMB_DEGREES, 1),
    "snow_cover": (native.COMB_SNOW_COVER, 0, 1),
    "xy_to_polar": (native.COMB_XY_TO_POLAR, 0, 2),
    "polar_to_xy": (native.COMB_POLAR_TO_XY, 0, 2),
    "r_to_d": (native.COMB_R_TO_D, 0, 1),
    "d_to_r": (native.COMB_D_TO_R, 0, 1),
    "q_to_r": (native.COMB_Q_TO_R, 0, 1),
    "r_to_q": (native.COMB_R_TO_Q, 0, 1),
    "q_to_r_level": (native.COMB_Q_TO_R, 0, 1),
    "r_to_q_level": (native.COMB_R_TO_Q, 0, 1),
    "q_to_d": (native.COMB_Q_TO_D, 0, 1),
    "d_to_q": (native.COMB_D_TO_Q, 0, 1),
}
LAYOUTS = [(COLUMNS, 0), (FIELDS, 0), (COLUMNS, 1), (FIELDS, 3)]  # (layout, padding of the pitch): the last two are not vector-aligned
LAYOUT_IDS = ["columns", "fields", "columns-pitch+1", "fields-pitch+3"]


def _stack(values: np.ndarray, layout: int, pad: int, dev) -> tuple[torch.Tensor, int]:
    """[n_lev, n_pts] values as a stack whose pitch is the row length + pad (padding: NaN); pad > 0 makes the pitch odd-sized."""
    n_lev, n_pts = values.shape
    rows, row_len = (n_pts, n_lev) if layout == COLUMNS else (n_lev, n_pts)
    per16 = 16 // values.itemsize
    pitch = row_len + pad if pad else -(-row_len // per16) * per16
    data = torch.full((rows, pitch), float("nan"), dtype=torch.float32 if values.dtype == np.float32 else torch.float64, device=dev)
    data[:, :row_len] = torch.from_numpy(np.ascontiguousarray(values.T if layout == COLUMNS else values)).to(dev)
    return data, pitch


def _values(data: torch.Tensor, layout: int, n_lev: int, n_pts: int) -> np.ndarray:
    a = data[:, : (n_lev if layout == COLUMNS else n_pts)].cpu().numpy()
    return a.T.copy() if layout == COLUMNS else a


def run_combine(op, flags, n_out, inputs, layout, pad, dev, levels=None):
    n_lev, n_pts = inputs[0].shape
    ins = [_stack(x, layout, pad, dev) for x in inputs]
    outs = [_stack(np.zeros_like(inputs[0]), layout, pad, dev) for _ in range(n_out)]
    lp = None if levels is None else torch.from_numpy(np.asarray(levels, dtype=np.float64)).to(dev)
    native.combine_stack(op, [d for d, _ in ins], [d for d, _ in outs], n_pts=n_pts, n_lev=n_lev, pitch=ins[0][1], layout=layout,
                         level_param=lp, flags=flags)
    return [_values(d, layout, n_lev, n_pts) for d, _ in outs]


def run_pointwise(op, x, layout, pad, dev):
    n_lev, n_pts = x.shape
    src, pitch = _stack(x, layout, pad, dev)
    dst, _ = _stack(np.zeros_like(x), layout, pad, dev)
    prog = native.level_program([[(op, 0, 0.0, 0.0)] * n_lev], dev)
    native.pointwise_stack(src, dst, n_pts=n_pts, n_lev=n_lev, x_pitch=pitch, y_pitch=pitch, layout=layout, prog=prog, n_stage=1)
    return [_values(dst, layout, n_lev, n_pts)]


def run_statement(st: X.Statement, layout, pad, dev):
    if st.name in ("exp", "log"):
        return run_pointwise(native.OP_EXP if st.name == "exp" else native.OP_LOG, st.inputs[0], layout, pad, dev)
    op, flags, n_out = COMB[st.name]
    return run_combine(op, flags, n_out, st.inputs, layout, pad, dev, levels=st.levels)


def _worst(err, st, where=None):
    mask = np.ones(err.size, bool) if where is None else where
    i = int(np.argmax(np.where(mask, err, -1.0)))
    return "at %s %s" % (st.case.reshape(-1)[i], [float(x.reshape(-1)[i]) for x in st.inputs])


def _same_specials(got, want, skip=None):
    """NaN positions and infinities as numpy's statement gives them.  (Zeros whose sign the statement defines are exact references and
    checked bit for bit by the ulp measure; a zero that comes out of a cancellation, like xy_to_polar's 360 - 360, is measured in ulps.)"""
    got, want = got.reshape(-1), want.reshape(-1)
    keep = np.ones(got.size, bool) if skip is None else ~skip
    assert np.array_equal(np.isnan(got[keep]), np.isnan(want[keep])), "NaN positions differ from numpy's"
    inf = keep & np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), "infinities differ from numpy's"


REPORT: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        print("\nmax ulps against exact arithmetic (kernel / numpy's own):")
        for (name, dt, out), (k, n, bound) in sorted(REPORT.items()):
            print(f"  {name:<13} out{out} {dt:<8} kernel {k:8.3f}   numpy {n:8.3f}   bound {bound}")


@pytest.mark.parametrize("layout,pad", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", X.SINGLE_FUNCTION)
def test_single_function_operators_within_budget(dev, name, dtype, layout, pad):
    st = X.statement(name, dtype)
    got = run_statement(st, layout, pad, dev)
    bud = budgets(dtype)
    for out, g in enumerate(got):
        assert g.dtype == dtype
        skip = st.alt[out][0] if out in st.alt else None
        _same_specials(g, st.numpy_out[out], skip)
        err = st.errors(out, g)
        bound = np.full(err.size, bud[(name, out)])
        if name.startswith("cos_sin") and dtype == np.float64 and FAST_SINCOS:  # beyond 1e5 the library's sincos
            bound[st.case.reshape(-1) == "beyond 1e5"] = LIB64["sincos"]
        k = float(err.max())
        key = (name, np.dtype(dtype).name, out)
        REPORT[key] = (max(k, REPORT.get(key, (0,))[0]), float(st.numpy_errors(out).max()), bud[(name, out)])
        bad = err > bound
        assert not bad.any(), f"{name} output {out}: {k:.3f} ulps > {bud[(name, out)]} ({int(bad.sum())} points) {_worst(err, st, bad)}"


@pytest.mark.parametrize("layout,pad", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", X.COMPOSED_STATEMENTS)
def test_composed_statements_no_worse_than_numpy(dev, name, dtype, layout, pad):
    st = X.statement(name, dtype)
    got = run_statement(st, layout, pad, dev)
    for out, g in enumerate(got):
        assert g.dtype == dtype
        skip = st.alt[out][0] if out in st.alt else None
        _same_specials(g, st.numpy_out[out], skip)
        err, ref = st.errors(out, g), st.numpy_errors(out)
        assert np.isfinite(err).all(), f"{name} output {out}: a special value against a finite exact one {_worst(err, st)}"
        ceiling = CEILING[name] if st.kinds[out] != X.SINGLE else budgets(dtype)[(name, out)]
        key = (name, np.dtype(dtype).name, out)
        REPORT[key] = (max(float(err.max()), REPORT.get(key, (0,))[0]), float(ref[np.isfinite(ref)].max()), ceiling)
        assert err.max() <= ceiling, f"{name} output {out}: {err.max():.3f} ulps > ceiling {ceiling} {_worst(err, st)}"
        if st.kinds[out] == X.SINGLE:  # the speed of xy_to_polar: a hypot
            continue
        for case in np.unique(st.case):
            m = st.case.reshape(-1) == case
            ok = m & np.isfinite(ref)
            if ok.any():
                assert err[ok].max() <= ref[ok].max() + SLACK, (
                    f"{name} output {out}, {case}: kernel {err[ok].max():.3f} ulps, numpy {ref[ok].max():.3f} {_worst(err, st, ok)}")


@pytest.mark.parametrize("layout,pad", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_arithmetic_operators_bit_exact(dev, dtype, layout, pad):
    """SNOW_DEPTH_M, SUB, SUM, W_TO_WZ, WZ_TO_W round once per operation in numpy's order: the oracle's bits, NaN, +-inf, +-0 and
    subnormals included (README: bit-exact arithmetic)."""
    a, b, c, d = (x.reshape(X.N_LEV, -1) for x in X.arithmetic_cases(dtype))
    w, t, q = (x.reshape(X.N_LEV, -1) for x in X.w_cases(dtype))
    levels = X.level_pressures(dtype, X.N_LEV)
    bits = np.int32 if dtype == np.float32 else np.int64

    def same(got, want, what):
        assert got.dtype == want.dtype == dtype, what
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what + ": NaN positions"
        diff = got[~nan].view(bits) != want[~nan].view(bits)
        assert not diff.any(), f"{what}: {int(diff.sum())} values differ, e.g. {got[~nan][diff][:3]} vs {want[~nan][diff][:3]}"

    with np.errstate(all="ignore"):
        same(run_combine(native.COMB_SNOW_DEPTH_M, 0, 1, [a, b], layout, pad, dev)[0], oracle.snow_depth_m(a, b), "snow_depth_m")
        same(run_combine(native.COMB_SUB, 0, 1, [a, b], layout, pad, dev)[0], oracle.interval_difference(a, b), "sub")
        want = np.stack([oracle.sum_fields([x[l].copy() for x in (a, b, c, d)]) for l in range(X.N_LEV)])
        same(run_combine(native.COMB_SUM, 0, 1, [a, b, c, d], layout, pad, dev)[0], want, "sum")
        want = np.stack([oracle.w_to_wz(w[l], t[l], q[l], dtype(levels[l])) for l in range(X.N_LEV)])
        same(run_combine(native.COMB_W_TO_WZ, 0, 1, [w, t, q], layout, pad, dev, levels=levels)[0], want, "w_to_wz")
        want = np.stack([oracle.wz_to_w(w[l], t[l], q[l], dtype(levels[l])) for l in range(X.N_LEV)])
        same(run_combine(native.COMB_WZ_TO_W, 0, 1, [w, t, q], layout, pad, dev, levels=levels)[0], want, "wz_to_w")
