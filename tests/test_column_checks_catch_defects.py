"""The checks of tests/test_gpu_column_ulps.py, run on the CPU against a stand-in of ``atx_pressure_at_height_stack`` — the restatement
reading the same five storage shapes — once as it is (every check passes) and once per planted defect (the check that is there for
it fails).  No deliberately broken kernel ever runs on a device; this is where each GPU assertion is seen to fail."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import exact_statements as X
import test_gpu_column_ulps as G
import vertical_restatement as vr

CPU = torch.device("cpu")


def stand_in(defect=None):
    """``native.pressure_at_height_stack`` on CPU tensors: the restatement's arithmetic, level by level as the kernel walks."""

    def kernel(t, q, sp, A, B, out, *, n_pts, n_lev, pitch, layout, height):
        n = n_lev

        def levels(x):
            a = x.numpy()
            assert a.shape[1] == pitch
            if defect == "padding read as a level" and layout == G.COLUMNS and pitch > n:  # level n - 1 taken one element too far
                return np.concatenate([a[:n_pts, : n - 1], a[:n_pts, n: n + 1]], axis=1).T.astype(np.float64)
            return (a[:n_pts, :n].T if layout == G.COLUMNS else a[:n, :n_pts]).astype(np.float64)

        tt, qq, s = levels(t), levels(q), sp.numpy()[:n_pts].astype(np.float64)
        with np.errstate(all="ignore"):
            p_full, p_half, alpha = vr.pressure_at_model_levels(A.numpy(), B.numpy(), s)
            if defect == "float32 log":
                ph = p_half
                alpha[1:] = 1.0 - ph[1:-1] / (ph[2:] - ph[1:-1]) * np.log((ph[2:] / ph[1:-1]).astype(np.float32)).astype(np.float64)
            term = alpha * (vr.RD * (1.0 - qq) + vr.RV * qq) * tt
            acc = np.float32 if defect == "float32 accumulation" else np.float64
            dphi = np.flip(np.cumsum(np.flip(term, axis=0).astype(acc), axis=0, dtype=acc), axis=0).astype(np.float64)
            tdphi = float(height) * vr.G
            counts = tdphi >= dphi if defect == ">= for >" else tdphi > dphi
            i = counts.sum(axis=0)
            a = n - i - 1
            a = np.where(a < 0, a + n, a)
            b = np.minimum(np.where(i == n, 0, a + 1), n - 1)
            if defect == "a, b shifted by one":
                mid = (i > 0) & (i < n)
                a, b = np.where(mid, np.maximum(a - 1, 0), a), np.where(mid, np.maximum(b - 1, 1 if n > 1 else 0), b)
            pick = lambda x, k: np.take_along_axis(x, k[np.newaxis, ...], axis=0)[0]  # noqa: E731
            da, db = pick(dphi, a), pick(dphi, b)
            if defect == "second walk one level off":
                walk = X.second_walk(dphi, tdphi)
                da = np.where(walk, pick(dphi, np.maximum(a - 1, 0)), da)
            below = p_half[n] + tdphi / dphi[n - 1] * (p_full[n - 1] - p_half[n])
            above = pick(p_full, b) + (tdphi - db) / (da - db) * (pick(p_full, a) - pick(p_full, b))
            res = np.where(i == 0, below, above)
            if defect == "route-dependent arithmetic" and layout == G.FIELDS:
                res = np.nextafter(res, np.inf)
            o = out.numpy()
            o[:n_pts] = res.astype(o.dtype)
            if defect == "writes one past the end":
                o[n_pts] = o[n_pts - 1]
            if defect == "modifies an input":
                sp.numpy()[0] += 1.0

    return kernel


def run_checks(kernel, dtype, n_lev, shapes=G.SHAPES, cases=None):
    st = X.column_statement(dtype, n_lev)
    hs = [h for h, _ in st.heights]
    per_shape = {}
    for shape in shapes:
        per_shape[shape] = {}
        for case, (t, q, sp) in st.cases.items():
            if cases is None or case in cases:
                got = G.run_case(kernel, CPU, t, q, sp, st.A, st.B, hs, shape)
                G.check_ulps(st, case, got)
                per_shape[shape][case] = got
    for case in per_shape[shapes[0]]:
        G.check_routes_agree({s: per_shape[s][case] for s in shapes}, case)


@pytest.mark.parametrize("n_lev", X.COLUMN_N_LEV)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_restatement_passes_every_check(dtype, n_lev):
    run_checks(stand_in(), dtype, n_lev)


# defect -> (dtype, n_lev, cases that must catch it, the assertion that does)
DEFECTS = {
    "float32 accumulation": (np.float32, 60, ("atmosphere",), "ulps >"),  # the float32 contract: 0.5 + C64 2^-29
    "float32 log": (np.float32, 137, ("standard profile",), "ulps >"),
    ">= for >": (np.float64, 3, ("specials",), "NaN positions"),  # dphi[n-1] == 0 at height 0: 0 >= 0 counts, and 0 / 0 is lost
    "a, b shifted by one": (np.float64, 60, ("standard profile",), "ulps >"),
    "second walk one level off": (np.float64, 137, ("bent",), "ulps >"),
    "padding read as a level": (np.float64, 3, ("atmosphere",), "NaN positions"),  # only NaN padding proves it
    "route-dependent arithmetic": (np.float64, 3, ("atmosphere",), "differs from"),
    "writes one past the end": (np.float64, 3, ("atmosphere",), "written beyond"),
    "modifies an input": (np.float32, 3, ("atmosphere",), "input stack was modified"),
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_check_catches_its_defect(defect):
    dtype, n_lev, cases, message = DEFECTS[defect]
    with pytest.raises(AssertionError, match=message):
        run_checks(stand_in(defect), dtype, n_lev, cases=cases)


@pytest.mark.parametrize("defect", ["float32 accumulation", "float32 log"])
def test_float64_rule_catches_lost_precision_too(defect):
    """2 x numpy + SLACK under the ceiling, on float64 columns near the ground: what rtol 2e-13 let through."""
    with pytest.raises(AssertionError, match="near ground: kernel"):
        run_checks(stand_in(defect), np.float64, 137, shapes=("columns",), cases=("standard profile",))


def test_ceilings_are_derived():
    """C64 is ceil(2 x numpy's pinned worst + SLACK), the float32 bound is below 0.501 ulp for every one of them, and near the ground on
    physical columns the float64 ceiling is single digits (n_lev == 2 are the reference's two thin bottom layers: 10 m lies between
    its full levels, and numpy itself is 244 ulps out there)."""
    for (n_lev, group), row in G.C64.items():
        assert row == tuple(G.c64(n_lev, group, cls) for cls in X.HEIGHT_CLASSES), (n_lev, group)
        assert all(0.5 + c * 2.0**-29 < 0.501 for c in row)
    assert max(G.C64[(n, X.PHYSICAL)][0] for n in (1, 3, 60, 137)) <= 10
