"""The three column-tile kernels (``atx_levels_interpolate``, ``atx_geopotential_on_model_levels``, ``atx_heights_interpolate``) at the limits of
their tile (csrc/atx_column_tile.hpp): the cases of ``column_tile_restatement.TILE_CASES`` — full tiles of 256 points with a last tile of
1 and of 255, tiles of one to four points, the 64 KiB budget up to the largest shape that is accepted, the heights kernel's variables
staged a chunk at a time — then rows that start beyond element 2^31 in both layouts, and ``vertical.interpolate_levels`` on a stack the
column kernel refuses.  tests/test_column_tile_host.py holds every case of the table to its regime without a GPU.

No comparison is new: the helpers, the canary checks and the rules are those of tests/test_gpu_levels.py (the restatement's bits for the
linear coordinate, ``levels_restatement.check_log`` for the log coordinate), tests/test_gpu_geopotential.py (``gr.check``) and
tests/test_gpu_heights.py (``hr.check``, every storage byte-identical to the others) — with numpy's pinned worst error of the class
where the host tests pin one, and numpy's worst on the case itself, measured on the CPU, where they do not.

Every case prints the restated plan — PT, budget, LDS bytes, tiles, chunk — next to what the kernel gave.  The figures of the heights
and log cases go to the reports of tests/test_gpu_heights.py and tests/test_gpu_levels.py (``ATX_HEIGHTS_ULPS_JSON``,
``ATX_LEVELS_ULPS_JSON``; profiles/heights_ulps.json, profiles/levels_ulps.json).
"""

from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import column_tile_restatement as ct
import geopotential_restatement as gr
import heights_restatement as hr
import levels_restatement as lr
import test_gpu_geopotential as on_geopotential
import test_gpu_heights as on_heights
import test_gpu_levels as on_levels
from anemoi_transform_amd import native_geopotential, native_heights, native_levels
from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack
from anemoi_transform_amd.vertical import interpolate_levels
from hybrid_column_common import CANARY
from test_geopotential_host import NUMPY_WORST_GEOPOTENTIAL
from test_heights_host import NUMPY_WORST_HEIGHTS

pytestmark = pytest.mark.gpu

CASES = {kernel: [c for c in ct.TILE_CASES if c.kernel == kernel] for kernel in (ct.LEVELS, ct.GEOPOTENTIAL, ct.HEIGHTS)}


def said(case: ct.TileCase) -> str:
    """The restated plan of the case, per storage where the storages differ."""
    plans = {storage: ct.PLANS[case.kernel](case.T, case.shape, ct.storage_of(case.kernel, storage)) for storage in case.storages}
    first = plans[case.storages[0]]
    assert first.budget is not None and (first.PT, first.budget) == (case.PT, case.budget)
    last = first.last_tile(ct.points_of(case.kernel, case.shape))
    text = f"{case.name} [{case.regime}]: PT {first.PT}, budget {first.budget}, tiles {first.tiles}, last tile {last}"
    return text + ", LDS bytes " + " / ".join(str(p.lds_bytes) for p in plans.values()) + ("" if first.chunk is None else ", chunk " + " / ".join(
        str(p.chunk) for p in plans.values()))


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The figures of this module alone, where it runs alone; in a run of the whole suite the two modules' own reports, which hold these
    figures too, are written after this one."""
    yield
    if on_heights.REPORT and os.environ.get("ATX_HEIGHTS_ULPS_JSON"):
        with open(os.environ["ATX_HEIGHTS_ULPS_JSON"], "w") as f:
            json.dump(dict(unit="ulps of max(|x[a]|, |x[b]|) in the stack's type", kernel=on_heights.REPORT), f, indent=1)
            f.write("\n")
    if on_levels.LOG_REPORT and os.environ.get("ATX_LEVELS_ULPS_JSON"):
        with open(os.environ["ATX_LEVELS_ULPS_JSON"], "w") as f:
            json.dump(on_levels.LOG_REPORT, f, indent=1)


# ---- the cases of the table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", CASES[ct.LEVELS], ids=lambda c: c.name)
def test_levels_at_the_limits_of_the_tile(dev, tile):
    """Linear: the restatement's bits under both policies in the three column storages.  Log: ``lr.check_log`` in each of them."""
    case = lr.shape_case(tile.T, *tile.shape)
    if tile.coordinate == lr.LOG:
        for storage in tile.storages:
            report: dict = {}
            lr.check_log(lambda c, coordinate, outside: on_levels.run_kernel(dev, c, storage, coordinate, outside), [case], report)
            for name, row in report.items():
                on_levels.LOG_REPORT[f"{name} {storage}"] = row
                print(f"{said(tile)} | {storage}: kernel {row['kernel']:.4f} ulps, numpy {row['numpy_float64']:.4f}, bound {row['bound']:.6g}")
        return
    for outside in (lr.NEAREST, lr.MISSING):
        want = lr.reference(case, lr.LINEAR, outside)
        for storage in tile.storages:
            lr.assert_same_bits(on_levels.run_kernel(dev, case, storage, lr.LINEAR, outside), want, f"{case.name} {storage} {outside}")
    print(f"{said(tile)} | the restatement's bits in {len(tile.storages)} storages, both policies")


@pytest.mark.parametrize("tile", CASES[ct.GEOPOTENTIAL], ids=lambda c: c.name)
def test_geopotential_at_the_limits_of_the_tile(dev, tile):
    n_lev, kind, n_pts, with_zs = tile.shape
    case = on_geopotential.expanded(gr.make_case(tile.T, n_lev, kind, with_zs), n_pts)
    first, report = None, {}
    for storage in on_geopotential.STORAGE:
        got = on_geopotential.run_kernel(dev, case, storage, n_pts)
        if first is None:
            gr.check(lambda c: got, [case], NUMPY_WORST_GEOPOTENTIAL, report)
            first = got
        else:
            assert got.tobytes() == first.tobytes(), f"{case.name}: {storage} differs from {on_geopotential.STORAGE[0]}"
    row = report[case.name]
    print(f"{said(tile)} | kernel {row['kernel']:.4f} ulps of U, numpy {row['numpy_float64']:.4f}, bound {row['bound']:.6g}")


def numpy_worst_of(case: hr.HeightsCase) -> float:
    """The class's pinned figure, or — a class the host test pins nothing for — numpy's worst on the case itself, on the CPU."""
    key = (case.n_lev, case.kind, case.reference)
    return NUMPY_WORST_HEIGHTS[key] if key in NUMPY_WORST_HEIGHTS else hr.numpy_worst(case)


@pytest.mark.parametrize("tile", CASES[ct.HEIGHTS], ids=lambda c: c.name)
def test_heights_at_the_limits_of_the_tile(dev, tile):
    """``hr.check`` under both policies; the three column storages, the mixed one and the two field-major ones byte for byte the same."""
    case = hr.make_case(tile.T, *tile.shape)
    assert on_heights.STORAGE[: len(tile.storages)] == ct.COLUMN_STORAGE + (on_heights.MIXED,)
    report: dict = {}
    hr.check(on_heights.every_storage(dev, case), [case], numpy_worst_of, report)
    on_heights.REPORT.update(report)
    row = report[case.name]
    print(f"{said(tile)} | kernel {row['kernel']:.4f} ulps, numpy {row['numpy_float64']:.4f}, bound {row['bound']:.8g}")


# ---- rows that start beyond element 2^31 ---------------------------------------------------------------------------------------------
BEYOND = 1 << 31
GUARD = 16  # the elements behind each written row that must keep the canary
LONG_PITCH = 1 << 20                 # x 2050 points, or x 2052 rows and more: beyond 2^31 elements
ROW_PITCH = (1 << 23) + (1 << 16)    # x the 255 rows above the last of a 256-level stack: beyond 2^31 elements (2^23 is not: 255 x 2^23 + 65 < 2^31)
MANY_POINTS, FEW_POINTS = 2050, 65


def need_memory(dev) -> None:
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 24 * 2**30:
        pytest.skip(f"two stacks beyond 2^31 float32 elements take 17 GiB; {free / 2**30:.1f} GiB of device memory are free")


def long_stack(dev, rows: int, row_len: int, pitch: int, values: np.ndarray | None = None) -> torch.Tensor:
    """``[rows, pitch]`` float32, uninitialised: the first ``row_len`` elements of every row hold ``values``, or, an output, the GUARD
    elements behind them the canary.  Nothing else is written."""
    assert (rows - 1) * pitch + row_len > BEYOND
    data = torch.empty((rows, pitch), dtype=torch.float32, device=dev)
    if values is None:
        data[:, row_len: row_len + GUARD] = CANARY
    else:
        data[:, :row_len] = torch.from_numpy(np.ascontiguousarray(values)).to(dev)
    return data


def tight(dev, values: np.ndarray | None, rows: int = 0, row_len: int = 0) -> torch.Tensor:
    if values is None:
        return torch.full((rows, row_len + GUARD), CANARY, dtype=torch.float32, device=dev)
    return torch.from_numpy(np.ascontiguousarray(values)).to(dev)


def taken(out: torch.Tensor, row_len: int, what: str) -> np.ndarray:
    """The first ``row_len`` elements of every row, after the GUARD elements behind them have been found untouched."""
    torch.cuda.synchronize()
    assert (out[:, row_len: row_len + GUARD] == CANARY).all().item(), f"{what}: written behind the {row_len} values of a row"
    return out[:, :row_len].cpu().numpy()


def up64(dev, a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def levels_beyond(dev, layout: int, shape: tuple, pitch: int) -> None:
    need_memory(dev)
    case = lr.shape_case(np.float32, *shape)
    n_pts, n_var, n_lev, n_tgt = case.n_pts, case.n_var, case.n_lev, case.n_tgt
    values = case.x.reshape(n_pts, n_var * n_lev)
    if layout == COLUMNS:
        src, out = long_stack(dev, n_pts, n_var * n_lev, pitch, values), long_stack(dev, n_pts, n_var * n_tgt, pitch)
        print("plan:", ct.levels_plan_of(np.float32, n_pts, n_lev, n_tgt, n_var, (True, pitch)))
    else:
        src, out = long_stack(dev, n_var * n_lev, n_pts, pitch, values.T), long_stack(dev, n_var * n_tgt, n_pts, pitch)
    sp = torch.from_numpy(case.sp).to(dev)
    for outside in (lr.NEAREST, lr.MISSING):
        native_levels.interpolate(src, out, sp, up64(dev, case.A), up64(dev, case.B), up64(dev, case.targets), n_pts=n_pts, n_var=n_var, n_lev=n_lev,
                                  n_tgt=n_tgt, src_pitch=pitch, out_pitch=pitch, layout=layout, outside=outside)
        got = taken(out, n_var * n_tgt if layout == COLUMNS else n_pts, case.name)
        got = got.reshape(n_pts, n_var, n_tgt) if layout == COLUMNS else np.ascontiguousarray(got.T).reshape(n_pts, n_var, n_tgt)
        lr.assert_same_bits(got, lr.reference(case, lr.LINEAR, outside), f"{case.name} pitch {pitch} {outside}")
    del src, out
    torch.cuda.empty_cache()


def test_levels_columns_beyond_two_to_the_31_elements(dev):
    """float32, pitch 2^20: the rows of points 2048 and 2049 start beyond element 2^31 in src and in out; nine tiles, the last of two points."""
    levels_beyond(dev, COLUMNS, (MANY_POINTS, 3, 5, 1), LONG_PITCH)


def test_levels_fields_beyond_two_to_the_31_elements(dev):
    """float32, pitch 2^20: 9 variables of 256 levels are 2304 source rows, 9 x 228 targets 2052 output rows — the last of both start
    beyond element 2^31."""
    levels_beyond(dev, FIELDS, (FEW_POINTS, 256, 228, 9), LONG_PITCH)


def geopotential_beyond(dev, layout: int, n_lev: int, n_pts: int, pitch: int) -> None:
    """t and out long with q tight, then q and out long with t tight: never more than two long stacks."""
    need_memory(dev)
    base = gr.make_case(np.float32, n_lev, gr.WHOLE, True)
    case = on_geopotential.expanded(base, n_pts)
    pinned = NUMPY_WORST_GEOPOTENTIAL if (n_lev, gr.WHOLE) in NUMPY_WORST_GEOPOTENTIAL else {(n_lev, gr.WHOLE): gr.numpy_worst(base)}  # on the CPU
    shape = (n_pts, n_lev) if layout == COLUMNS else (n_lev, n_pts)
    t, q = (case.t, case.q) if layout == COLUMNS else (case.t.T, case.q.T)
    sp, zs = torch.from_numpy(case.sp).to(dev), torch.from_numpy(case.zs).to(dev)
    if layout == COLUMNS:
        print("plan:", [ct.geo_plan_of(np.float32, n_pts, n_lev, *forms) for forms in (((True, pitch), (True, n_lev)), ((True, n_lev), (True, pitch)))])
    results = []
    for long_one in ("t", "q"):
        out = long_stack(dev, *shape, pitch)
        ts = long_stack(dev, *shape, pitch, t) if long_one == "t" else tight(dev, t)
        qs = long_stack(dev, *shape, pitch, q) if long_one == "q" else tight(dev, q)
        native_geopotential.geopotential(ts, qs, sp, zs, up64(dev, case.A), up64(dev, case.B), out, n_pts=n_pts, n_lev=n_lev, t_pitch=ts.stride(0),
                                         q_pitch=qs.stride(0), out_pitch=pitch, layout=layout)
        got = taken(out, shape[1], f"{case.name} long {long_one}")
        results.append(got if layout == COLUMNS else np.ascontiguousarray(got.T))
        del out, ts, qs
        torch.cuda.empty_cache()
    gr.check(lambda c: results[0], [case], pinned)
    assert results[1].tobytes() == results[0].tobytes()


def test_geopotential_columns_beyond_two_to_the_31_elements(dev):
    geopotential_beyond(dev, COLUMNS, 3, MANY_POINTS, LONG_PITCH)


def test_geopotential_fields_beyond_two_to_the_31_elements(dev):
    """256 levels: the last row alone starts beyond element 2^31, at a pitch a little over 2^23."""
    geopotential_beyond(dev, FIELDS, 256, FEW_POINTS, ROW_PITCH)


def heights_beyond(dev, layout: int, shape: tuple, pitch: int, tq_pitch: int) -> None:
    """src and out long with t and q tight, then t and q long with src and out tight — under both policies, through ``hr.check``."""
    need_memory(dev)
    case = hr.make_case(np.float32, *shape)
    n_pts, n_var, n_lev, n_tgt = case.n_pts, case.n_var, case.n_lev, case.n_tgt
    rows = dict(src=n_var * n_lev, t=n_lev, q=n_lev, out=n_var * n_tgt)
    values = dict(src=case.x.reshape(n_pts, -1), t=case.per_point(case.geo.t), q=case.per_point(case.geo.q))
    sp = torch.from_numpy(case.per_point(case.geo.sp)).to(dev)
    zs = torch.from_numpy(case.per_point(case.zs)).to(dev) if case.reference == hr.SEA else None
    if layout == COLUMNS:
        print("plan:", ct.heights_plan_of(np.float32, n_pts, n_lev, n_tgt, n_var, (True, pitch), (True, ct.storage_form("columns", n_lev, np.float32)[1]),
                                          (True, ct.storage_form("columns", n_lev, np.float32)[1])))
    results: dict = {}
    for long_ones, long_pitch in ((("src", "out"), pitch), (("t", "q"), tq_pitch)):
        stacks = {}
        for name in ("src", "t", "q", "out"):
            shape2 = (n_pts, rows[name]) if layout == COLUMNS else (rows[name], n_pts)
            held = None if name == "out" else (values[name] if layout == COLUMNS else values[name].T)
            stacks[name] = long_stack(dev, *shape2, long_pitch, held) if name in long_ones else tight(dev, held, *shape2)
        for outside in (hr.NEAREST, hr.MISSING):
            native_heights.interpolate(stacks["src"], stacks["out"], stacks["t"], stacks["q"], sp, zs, up64(dev, case.geo.A), up64(dev, case.geo.B),
                                       up64(dev, case.targets), n_pts=n_pts, n_var=n_var, n_lev=n_lev, n_tgt=n_tgt, src_pitch=stacks["src"].stride(0),
                                       t_pitch=stacks["t"].stride(0), q_pitch=stacks["q"].stride(0), out_pitch=stacks["out"].stride(0), layout=layout,
                                       reference=case.reference, outside=outside)
            got = taken(stacks["out"], rows["out"] if layout == COLUMNS else n_pts, f"{case.name} long {long_ones} {outside}")
            got = got.reshape(n_pts, n_var, n_tgt) if layout == COLUMNS else np.ascontiguousarray(got.T).reshape(n_pts, n_var, n_tgt)
            results.setdefault(outside, []).append(got)
        del stacks
        torch.cuda.empty_cache()
    for outside, (first, second) in results.items():
        assert second.tobytes() == first.tobytes(), f"{case.name} {outside}: long t and q differ from long src and out"
    report: dict = {}
    hr.check(lambda c, outside: results[outside][0], [case], numpy_worst_of, report)
    on_heights.REPORT.update(report)


def test_heights_columns_beyond_two_to_the_31_elements(dev):
    """The thirteen heights: three levels above the ground bracket the higher ones."""
    heights_beyond(dev, COLUMNS, (MANY_POINTS, 3, hr.WHOLE, 13, 1, hr.GROUND), LONG_PITCH, LONG_PITCH)


def test_heights_fields_beyond_two_to_the_31_elements(dev):
    """2304 source rows and 2052 output rows at pitch 2^20; then the 256 rows of t and of q at a pitch a little over 2^23.  17 points:
    the exact statement of 65 x 9 x 228 elements takes the CPU six seconds."""
    heights_beyond(dev, FIELDS, (17, 256, hr.WHOLE, 228, 9, hr.GROUND), LONG_PITCH, ROW_PITCH)


# ---- interpolate_levels past the limit of the column kernel --------------------------------------------------------------------------
def test_interpolate_levels_splits_the_variables_the_column_kernel_refuses(dev, monkeypatch):
    """56 float64 variables of 137 levels, one more than the largest stack the restatement accepts: the column kernel refuses them and
    ``interpolate_levels`` launches halves — the restatement's bits under both policies, the bits of every variable launched alone, and of
    the field-major kernel, which takes the whole stack in one call; 54 variables are one call."""
    n_var, n_pts = 56, 9
    assert ct.levels_plan(np.float64, (n_pts, 137, 13, n_var)).refused and not ct.levels_plan(np.float64, (n_pts, 137, 13, 54)).refused
    case = lr.shape_case(np.float64, n_pts, 137, 13, n_var)
    stack = Stack.from_fields(list(case.x.reshape(n_pts, -1).T), dev=dev, layout=COLUMNS)
    sp = torch.from_numpy(case.sp).to(dev)
    launches = []
    real = native_levels.interpolate

    def counted(*a, **k):
        launches.append(k["n_var"])
        return real(*a, **k)

    monkeypatch.setattr(native_levels, "interpolate", counted)
    as_case = lambda out, count: np.ascontiguousarray(out.numpy().T).reshape(n_pts, count, 13)  # noqa: E731
    for outside in (lr.NEAREST, lr.MISSING):
        del launches[:]
        got = as_case(interpolate_levels(stack, sp, case.A, case.B, case.targets, n_var=n_var, outside=outside), n_var)
        assert launches == [56, 28, 28], launches  # the refused call, then its halves
        lr.assert_same_bits(got, lr.reference(case, lr.LINEAR, outside), f"{case.name} split {outside}")
        del launches[:]
        fields = as_case(interpolate_levels(stack.to_layout(FIELDS), sp, case.A, case.B, case.targets, n_var=n_var, outside=outside), n_var)
        assert launches == [56] and fields.tobytes() == got.tobytes()
        del launches[:]
        fewer = as_case(interpolate_levels(Stack(stack.data, n_pts, 54 * 137, COLUMNS), sp, case.A, case.B, case.targets, n_var=54, outside=outside), 54)
        assert launches == [54] and fewer.tobytes() == got[:, :54].tobytes()
        for v in range(n_var):
            alone = as_case(interpolate_levels(Stack(stack.data[:, v * 137:], n_pts, 137, COLUMNS), sp, case.A, case.B, case.targets, outside=outside), 1)
            assert alone.tobytes() == got[:, v: v + 1].tobytes(), (outside, v)
    print("56 x 137 float64 rows:", ct.levels_plan(np.float64, (n_pts, 137, 13, n_var)), "-> launches of 28 and 28:",
          ct.levels_plan(np.float64, (n_pts, 137, 13, 28)))
