"""The tile plan of the column-tile kernels without a GPU: the restatement (tests/column_tile_restatement.py) against the libraries' own
refusal messages — a refusal comes after validation and before any launch, and its message prints the LDS one point needs, so the
restated carve is held to the library's byte for byte at shapes where the library can be called without a device; the geopotential
kernel's refusal, which no shape reaches; the case table of the GPU test (tests/test_gpu_column_tile.py), every entry recomputed and held
to the regime it is there for; the tiles the suites of the three kernels reached before that table; and the variables of
``vertical.interpolate_levels`` split after a refusal, with a stand-in for the launch.
"""

from __future__ import annotations

import ctypes
import re

import numpy as np
import pytest

from anemoi_transform_amd import native, native_heights, native_levels

import column_tile_restatement as ct
import geopotential_restatement as gr
import heights_restatement as hr
import levels_restatement as lr
from hybrid_column_common import WIDTHS

ROUTES = ("vector", "scalar")
MESSAGE = re.compile(r"need (\d+) bytes of LDS, a workgroup has (\d+)")


def at(address: int) -> ctypes.c_void_p:
    return ctypes.c_void_p(address)  # never dereferenced: the call is refused before the launch


def form(route: str, rows: int, T) -> tuple[bool, int]:
    """``(aligned, pitch)`` of a stack on the route: the 16-byte route tight; the scalar route an odd pitch AND a base one element off."""
    if route == "vector":
        return ct.storage_form("columns", rows, T)
    return False, ct.storage_form("columns", rows, T)[1] + 1


def base(address: int, aligned: bool, T) -> ctypes.c_void_p:
    return at(address + (0 if aligned else np.dtype(T).itemsize))


# ---- the restatement against the library, at refusals --------------------------------------------------------------------------------
def levels_refusal(T, route: str, n_lev: int, n_tgt: int, n_var: int, n_pts: int = 9) -> tuple[int, str, ct.Plan]:
    src = form(route, n_var * n_lev, T)
    plan = ct.levels_plan_of(T, n_pts, n_lev, n_tgt, n_var, src)
    assert plan.refused, ("the call would launch", T, route, n_lev, n_tgt, n_var, plan)
    lib = native_levels.load()
    code = lib.atx_levels_interpolate(base(1 << 30, src[0], T), at(2 << 30), at(16), at(48), at(64), None, at(80), n_pts, n_var, n_lev, n_tgt, n_lev + 1,
                                      src[1], n_var * n_tgt, 0 if T is np.float32 else 1, native.COLUMNS, 0, 0, None)
    return code, lib.atx_levels_last_error().decode(), plan


def heights_refusal(T, route: str, n_lev: int, n_tgt: int, n_var: int, n_pts: int = 9) -> tuple[int, str, ct.Plan]:
    src, tq = form(route, n_var * n_lev, T), form(route, n_lev, T)
    plan = ct.heights_plan_of(T, n_pts, n_lev, n_tgt, n_var, src, tq, tq)
    assert plan.refused, ("the call would launch", T, route, n_lev, n_tgt, n_var, plan)
    lib = native_heights.load()
    # the stacks far apart: the overlap check passes
    code = lib.atx_heights_interpolate(base(1 << 40, src[0], T), at(2 << 40), base(3 << 40, tq[0], T), base(4 << 40, tq[0], T), at(16), at(32), at(48),
                                       at(64), at(80), n_pts, n_var, n_lev, n_tgt, n_lev + 1, src[1], tq[1], tq[1], n_var * n_tgt,
                                       0 if T is np.float32 else 1, native.COLUMNS, 1, 0, None)
    return code, lib.atx_heights_last_error().decode(), plan


def assert_refused_as_restated(code: int, message: str, plan: ct.Plan, what) -> None:
    assert code == native.ENOTIMPL, (what, code, message)
    found = MESSAGE.search(message)
    assert found, (what, message)
    print(f"{what}: restated bytes(1) {plan.lds_bytes}; the library: {message}")
    assert int(found.group(1)) == plan.lds_bytes, (what, message, plan.lds_bytes)
    assert int(found.group(2)) == ct.LDS_LIMIT, (what, message)


def test_the_constants_are_the_headers():
    assert (ct.BLOCK, ct.MAX_POINTS) == (256, 256) and ct.LDS_PREFERRED < ct.LDS_LIMIT
    assert ct.LDS_PREFERRED % 16 == 0 and ct.LDS_LIMIT % 16 == 0


def levels_boundary(T, route: str) -> int:
    n_lev, n_tgt = ct.LEVELS_BOUNDARY["n_lev"], ct.LEVELS_BOUNDARY["n_tgt"]
    return ct.first_refused(lambda n_var: ct.levels_plan_of(T, 9, n_lev, n_tgt, n_var, form(route, n_var * n_lev, T)), 1, 65535 // n_lev)


def heights_boundary(T, route: str) -> int:
    n_lev = ct.HEIGHTS_BOUNDARY["n_lev"]
    return ct.first_refused(lambda n_tgt: ct.heights_plan_of(T, 9, n_lev, n_tgt, 1, form(route, n_lev, T), form(route, n_lev, T), form(route, n_lev, T)),
                            1, 65536)


# (n_lev, n_tgt, n_var) well past the boundary, with other n_lev: every term of the carve carries weight in one of them
LEVELS_BEYOND = ((256, 64, 200), (1, 5000, 3), (61, 250, 261))
HEIGHTS_BEYOND = ((137, 6000, 2), (256, 20001, 1), (2, 4999, 13))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("T", WIDTHS)
def test_levels_refuses_with_the_restated_bytes_of_one_point(T, route):
    """The smallest refused n_var at 137 levels to 13 targets, by the restatement's search — the one before it is accepted by the
    restatement (the GPU test launches it) — and three shapes well past it."""
    n_lev, n_tgt = ct.LEVELS_BOUNDARY["n_lev"], ct.LEVELS_BOUNDARY["n_tgt"]
    first = levels_boundary(T, route)
    accepted = ct.levels_plan_of(T, 9, n_lev, n_tgt, first - 1, form(route, (first - 1) * n_lev, T))
    assert (accepted.PT, accepted.budget) == (1, ct.LDS_LIMIT) and ct.LDS_LIMIT - 16 * 69 < accepted.lds_bytes <= ct.LDS_LIMIT
    assert_refused_as_restated(*levels_refusal(T, route, n_lev, n_tgt, first), ("levels", T.__name__, route, first))
    for n_lev, n_tgt, n_var in LEVELS_BEYOND:
        code, message, plan = levels_refusal(T, route, n_lev, n_tgt, n_var)
        assert_refused_as_restated(code, message, plan, ("levels", T.__name__, route, n_lev, n_tgt, n_var))
        assert f"one point's {n_var * n_lev} rows, {n_lev} levels and {n_tgt} targets" in message and "(split the variables)" in message


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("T", WIDTHS)
def test_heights_refuses_with_the_restated_bytes_of_one_point(T, route):
    """The smallest refused n_tgt at 3 levels, and three shapes well past it.  The carve does not depend on n_var: (2, 4999, 13) says so."""
    n_lev = ct.HEIGHTS_BOUNDARY["n_lev"]
    first = heights_boundary(T, route)
    tq = form(route, n_lev, T)
    accepted = ct.heights_plan_of(T, 9, n_lev, first - 1, 1, tq, tq, tq)
    assert (accepted.PT, accepted.budget, accepted.chunk) == (1, ct.LDS_LIMIT, 1) and ct.LDS_LIMIT - 16 <= accepted.lds_bytes <= ct.LDS_LIMIT
    assert_refused_as_restated(*heights_refusal(T, route, n_lev, first, 1), ("heights", T.__name__, route, first))
    for n_lev, n_tgt, n_var in HEIGHTS_BEYOND:
        code, message, plan = heights_refusal(T, route, n_lev, n_tgt, n_var)
        assert_refused_as_restated(code, message, plan, ("heights", T.__name__, route, n_lev, n_tgt, n_var))
        assert f"one point's {n_lev} levels and {n_tgt} targets" in message
        assert plan.lds_bytes == heights_refusal(T, route, n_lev, n_tgt, 1)[2].lds_bytes


def test_the_boundaries_are_those_of_the_case_table():
    """The searches behind ``TILE_CASES``' largest accepted shapes are the ones the refusals above were held to (the 16-byte route)."""
    for T in (np.float32, np.float64):
        assert ct.levels_first_refused(T) == levels_boundary(T, "vector") and ct.heights_first_refused(T) == heights_boundary(T, "vector")
    assert ct.levels_first_refused(np.float64) == 55 and ct.levels_first_refused(np.float32) == 110  # a dozen params fit; 55 float64 ones do not
    print("first refused: levels n_var", {T.__name__: ct.levels_first_refused(T) for T in (np.float32, np.float64)},
          "heights n_tgt", {T.__name__: ct.heights_first_refused(T) for T in (np.float32, np.float64)})


def test_the_geopotential_kernel_never_leaves_the_preferred_budget():
    """At the 256 levels of one call — the most the entry point takes — one point needs less than ``kTileLdsPreferred`` in both widths
    and on every route of t and of q: ``tile_points`` finds a tile under the first budget, so NO shape reaches the kernel's refusal
    (nor its 64 KiB budget), and there is no refused call to hold the restated ``geo_carve`` to.  The carve grows with n_lev, so the
    levels below 256 need less."""
    for T in (np.float32, np.float64):
        worst = 0
        for n_lev in range(1, 257):
            for t in ROUTES:
                for q in ROUTES:
                    plan = ct.geo_plan_of(T, 9, n_lev, form(t, n_lev, T), form(q, n_lev, T))
                    one = ct.geo_carve(1, ct.column_route(*form(t, n_lev, T), n_lev, ct.vec(T))[1], ct.column_route(*form(q, n_lev, T), n_lev, ct.vec(T))[1],
                                       np.dtype(T).itemsize, n_lev)
                    assert one < ct.LDS_PREFERRED and plan.budget == ct.LDS_PREFERRED and plan.PT >= 1, (T, n_lev, t, q, one)
                    worst = max(worst, one)
        print(f"geopotential {T.__name__}: one point needs at most {worst} bytes")
        assert worst == {np.float32: 10320, np.float64: 8240}[T]


# ---- the regime table ------------------------------------------------------------------------------------------------------------
def plans_of(case: ct.TileCase) -> dict:
    return {storage: ct.PLANS[case.kernel](case.T, case.shape, ct.storage_of(case.kernel, storage)) for storage in case.storages}


@pytest.mark.parametrize("case", ct.TILE_CASES, ids=lambda c: c.name)
def test_every_case_of_the_table_lands_in_its_regime(case):
    n_pts = ct.points_of(case.kernel, case.shape)
    for i, (storage, plan) in enumerate(plans_of(case).items()):
        what = (case.name, storage, plan)
        chunk = case.chunk[i] if isinstance(case.chunk, tuple) else case.chunk
        assert (plan.PT, plan.budget, plan.last_tile(n_pts), plan.chunk) == (case.PT, case.budget, case.last, chunk), what
        assert plan.lds_bytes <= plan.budget and plan.tiles == -(-n_pts // plan.PT), what
        if case.regime == ct.CAP:
            assert plan.PT == ct.MAX_POINTS == ct.BLOCK and plan.tiles > 1 and plan.last_tile(n_pts) in (1, ct.MAX_POINTS - 1), what
        elif case.regime == ct.SMALL:
            assert plan.PT <= 4 and plan.budget == ct.LDS_PREFERRED and plan.tiles >= 3, what
        elif case.regime in (ct.WIDE, ct.LARGEST):
            assert plan.budget == ct.LDS_LIMIT and plan.lds_bytes > ct.LDS_PREFERRED and plan.PT <= 2, what
        elif case.regime == ct.CHUNKS:
            n_lev, n_var = case.shape[1], case.shape[4]
            assert 3 * plan.chunk <= n_var and n_lev % 2 == 1, what
            if storage == "columns":  # src on the 16-byte route: a later chunk starts inside a vector, lead != 0
                assert any((v0 * n_lev) % ct.vec(case.T) for v0 in range(plan.chunk, n_var, plan.chunk)), what
        if case.regime == ct.LARGEST:  # one more along the axis is refused, in this storage too
            shape = list(case.shape)
            shape[3] += 1
            assert ct.PLANS[case.kernel](case.T, tuple(shape), ct.storage_of(case.kernel, storage)).refused, what


def test_the_table_holds_every_regime_the_kernels_have():
    have = {(c.kernel, np.dtype(c.T).name, c.regime) for c in ct.TILE_CASES}
    for T in ("float32", "float64"):
        for kernel in (ct.LEVELS, ct.HEIGHTS):
            assert {(kernel, T, r) for r in (ct.CAP, ct.SMALL, ct.WIDE, ct.LARGEST)} <= have | {(ct.LEVELS, "float32", ct.WIDE)}, (kernel, T)
            assert {c.last for c in ct.TILE_CASES if (c.kernel, np.dtype(c.T).name, c.regime) == (kernel, T, ct.CAP)} == {1, 255}
        assert (ct.HEIGHTS, T, ct.CHUNKS) in have and (ct.GEOPOTENTIAL, T, ct.CAP) in have
    assert {c.PT for c in ct.TILE_CASES if c.kernel == ct.LEVELS and c.regime in (ct.SMALL, ct.WIDE)} == {1, 2, 3, 4}
    assert {c.regime for c in ct.TILE_CASES if c.coordinate == "log"} == {ct.SMALL, ct.WIDE}
    assert len({c.name for c in ct.TILE_CASES}) == len(ct.TILE_CASES)
    # (float32 levels leave the preferred budget at 52 variables of 137 levels: its 64 KiB case is the largest accepted one)
    assert (ct.LEVELS, "float32", ct.LARGEST) in have


def reached(plan, shapes, points) -> tuple:
    """``(smallest PT, largest PT, budgets)`` over the shapes in both widths and the three column storages, of the launches of MORE THAN
    ONE tile, and the largest PT a single tile ran at."""
    many, budgets, single = [], set(), []
    for T in (np.float32, np.float64):
        for shape in shapes:
            for storage in ct.COLUMN_STORAGE:
                p = plan(T, shape, storage)
                if points(shape) == 0:
                    continue
                budgets.add(p.budget)
                (many if p.tiles > 1 else single).append(p.PT)
    return min(many), max(many), budgets, max(single)


def test_the_tiles_the_levels_suite_reached_before_this_table():
    """``levels_restatement.SHAPES`` and the edge cases (257 x 17 to 16 targets and 65 x 17 to 13, three variables): several tiles only
    from 6 to 134 points, the cap only with ONE point in one tile, nothing beyond 32 KiB."""
    shapes = lr.SHAPES + ((257, 17, 16, 3), (65, 17, 13, 3))
    assert reached(ct.levels_plan, shapes, lambda s: s[0]) == (6, 134, {ct.LDS_PREFERRED}, 256)


def test_the_tiles_the_heights_suite_reached_before_this_table():
    """``heights_restatement.SHAPES`` and the 65-point cases of 1 and 17 levels: several tiles only from 5 to 64 points; the tiles of
    106 points and more hold the whole field; nothing beyond 32 KiB."""
    shapes = hr.SHAPES + ((65, 1, hr.WHOLE, 13, 2, hr.SEA), (65, 17, hr.WHOLE, 13, 2, hr.SEA))
    assert reached(ct.heights_plan, shapes, lambda s: s[0]) == (5, 64, {ct.LDS_PREFERRED}, 256)


def test_the_tiles_the_geopotential_suite_reached_before_this_table():
    """``geopotential_restatement.SHAPES``: 9 to 256 points, the one kernel with several full tiles at the cap — (2, SUBSET, 257) and
    (3, WHOLE, 513), a last tile of one point; none of 255."""
    assert reached(ct.geo_plan, gr.SHAPES, lambda s: s[2]) == (9, 256, {ct.LDS_PREFERRED}, 256)
    plans = [(s, ct.geo_plan(np.float32, s)) for s in gr.SHAPES]
    capped = [(s, p.last_tile(s[2])) for s, p in plans if p.PT == 256 and p.tiles > 1]
    assert capped == [((2, gr.SUBSET, 257, True), 1), ((3, gr.WHOLE, 513, True), 1)]


# ---- vertical.interpolate_levels splits the variables after a refusal ----------------------------------------------------------------
def split_calls(monkeypatch, n_var: int, most: int, layout=native.COLUMNS, n_lev: int = 3, n_tgt: int = 2, n_pts: int = 4):
    """``interpolate_levels`` on a host stack with a stand-in for the launch that refuses more than ``most`` variables, as the library
    does: ``[(n_var, first source row, first output row, src_pitch, out_pitch)]`` of every call, refused ones included, and the result."""
    import torch

    from anemoi_transform_amd.stack import Stack
    from anemoi_transform_amd.vertical import interpolate_levels

    calls = []

    def stand_in(src, out, sp, A, B, targets, *, n_var, src_pitch, out_pitch, **kwargs):
        calls.append((n_var, src, out, src_pitch, out_pitch, kwargs))
        if n_var > most:
            raise NotImplementedError("atx_levels_interpolate: one point's rows need more bytes of LDS than a workgroup has (split the variables)")
        if layout == native.COLUMNS:
            out[:, : n_var * kwargs["n_tgt"]] = 1.0 + len(calls)

    monkeypatch.setattr(native_levels, "interpolate", stand_in)
    rows = n_var * n_lev
    data = torch.zeros((n_pts, rows + 1) if layout == native.COLUMNS else (rows, n_pts), dtype=torch.float64)
    stack = Stack(data, n_pts, rows, layout)
    out = interpolate_levels(stack, torch.zeros(n_pts), np.zeros(n_lev + 1), np.zeros(n_lev + 1), [5e4, 7e4][:n_tgt], n_var=n_var, outside="missing")
    elem = data.element_size()
    seen = []
    for count, src, dst, sp_, op_, kwargs in calls:
        assert (kwargs["n_pts"], kwargs["n_lev"], kwargs["n_tgt"], kwargs["layout"], kwargs["outside"]) == (n_pts, n_lev, n_tgt, layout, native_levels.MISSING)
        assert (sp_, op_) == (stack.pitch, out.pitch)  # the views keep the pitch
        seen.append((count, (src.data_ptr() - data.data_ptr()) // elem, (dst.data_ptr() - out.data.data_ptr()) // elem))
    return seen, out


def test_a_refused_column_stack_is_halved_down_to_what_is_accepted(monkeypatch):
    """Seven variables, at most two per launch: the order of the calls and the rows their views start at.  A refused call is followed
    by its two halves, the smaller first; each launch writes its own rows of the ONE output stack."""
    seen, out = split_calls(monkeypatch, 7, 2)
    assert seen == [(7, 0, 0), (3, 0, 0), (1, 0, 0), (2, 3, 2), (4, 9, 6), (2, 9, 6), (2, 15, 10)]  # (n_var, source row, output row): 3 levels, 2 targets
    assert (out.n_pts, out.n_lev, out.layout) == (4, 14, native.COLUMNS)
    written = out.data[:, :14]
    assert [float(v) for v in written[0]] == [4.0] * 2 + [5.0] * 4 + [7.0] * 4 + [8.0] * 4  # launches 3, 4, 6 and 7 of the list above
    # what is accepted at once is one call, whatever the layout; the field-major kernel has no tile and is never split
    assert split_calls(monkeypatch, 7, 7)[0] == [(7, 0, 0)]
    assert split_calls(monkeypatch, 7, 7, native.FIELDS)[0] == [(7, 0, 0)]
    with pytest.raises(NotImplementedError, match="split the variables"):
        split_calls(monkeypatch, 7, 2, native.FIELDS)


def test_a_single_variable_that_is_refused_raises(monkeypatch):
    """Nothing accepts: 5 variables, their first half of 2, its first half of 1 — which re-raises the library's refusal, and nothing follows."""
    import torch

    from anemoi_transform_amd.stack import Stack
    from anemoi_transform_amd.vertical import interpolate_levels

    counts = []

    def refuse(*args, n_var, **kwargs):
        counts.append(n_var)
        raise NotImplementedError(f"refused {n_var}")

    monkeypatch.setattr(native_levels, "interpolate", refuse)
    stack = Stack(torch.zeros(4, 16, dtype=torch.float64), 4, 15, native.COLUMNS)
    with pytest.raises(NotImplementedError, match="refused 1"):
        interpolate_levels(stack, torch.zeros(4), np.zeros(4), np.zeros(4), [5e4], n_var=5)
    assert counts == [5, 2, 1]
    del counts[:]
    with pytest.raises(NotImplementedError, match="refused 1"):
        interpolate_levels(Stack(stack.data, 4, 3, native.COLUMNS), torch.zeros(4), np.zeros(4), np.zeros(4), [5e4])
    assert counts == [1]
