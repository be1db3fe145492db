"""Model levels to height levels on the device: ``atx_heights_interpolate`` against the restatement of include/atx_heights.h
(tests/heights_restatement.py) — NaN and infinities exactly where the restatement has them, what the statement copies (above the top
level, the lowest half layer, below the ground) bit for bit, every finite interior value within the class's bound of the exact
statement, every storage shape byte-identical to the others, nothing written outside a point's rows, no input modified — then
``vertical.interpolate_to_heights`` and the ``ml_to_hl`` filter.

The accuracy rule is the project's rule for a kernel with a logarithm (``levels_restatement.log_budget``) with numpy's PINNED worst error
of the class (tests/test_heights_host.py::NUMPY_WORST_HEIGHTS), in ulps of max(|x[a]|, |x[b]|).  float64: 2 x worst + SLACK, SLACK = 2.0 —
kernel and numpy evaluate the same statements in the same order with IEEE operations, the one primitive that differs is the logarithm
(the library's is budgeted at 1 ulp, glibc's is at about half that), so the kernel may carry up to twice numpy's share.  float32:
0.5 + (2 x worst + SLACK) 2^-29 — the float64 arithmetic under that bound (one float64 ulp is 2^-29 float32 ulps) and one rounding at the
store, 0.5 ulp of y, which is at most 0.5 ulp of max(|x[a]|, |x[b]|) wherever w is inside [0, 1].  That is the rule's precondition: the
column's c never increases towards the ground, so that y lies inside its bracket — true of every case here but the bent one, which is
held to the float64 rule alone.  The brackets themselves are the exact ones: the host test asserts, in exact arithmetic, that every
target is at least 1e-9 |G| from every c[k] of its point.

Worst distance from exact measured on an MI355X (profiles/heights_ulps.json): float64 1833.94 ulps for the whole 137 levels above the
ground (numpy's own arithmetic: 1833.94, bound 3669.88), 1596.52 for the lowest 137 of 145 above the sea (bound 3195.04), 213.58 for 60
levels, 30.98 for 17, 6.00 for two, 0.80 for three; float32 at most 0.5000 (bound 0.5 + 2^-29 of the float64 ceiling) — the same bytes
in every storage shape; the geopotential kernel's output interpolated back to its targets: 0.00 ulps.

The test prints the figures of its run and writes them as JSON to the file that ``ATX_HEIGHTS_ULPS_JSON`` names, if it is set
(profiles/heights_ulps.json).
"""

from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import geopotential_restatement as gr
import heights_restatement as hr
from anemoi_transform_amd import native_geopotential, native_heights
from anemoi_transform_amd.fields import FieldList, fieldlist_from_dicts, new_field_from_stack
from anemoi_transform_amd.filters import create_filter_by_name
from anemoi_transform_amd.grids import lookup
from anemoi_transform_amd.stack import COLUMNS, FIELDS, Stack
from anemoi_transform_amd.vertical import interpolate_to_heights
from hybrid_column_common import CANARY, COLUMN_STORAGE, FIELD_STORAGE, WIDTHS, allocate
from test_heights_host import NUMPY_WORST_HEIGHTS

pytestmark = pytest.mark.gpu

# the storages it shares with the levels test, and between them t on the 16-byte route, q at an odd pitch and src one element off
MIXED = "columns-t-aligned-q-pitch+1-src-base+1"
STORAGE = COLUMN_STORAGE + (MIXED,) + FIELD_STORAGE


def take(data: torch.Tensor, n: int, what: str) -> np.ndarray:
    """The first ``n`` elements of every row of a pitched view as a host array — after asserting that everything else of the allocation
    it is a view of (the rest of the pitch, the elements before and behind the view) still holds CANARY."""
    base = data._base if data._base is not None else data
    host = base.cpu().numpy().copy().reshape(-1)
    rows, pitch = data.shape
    off = (data.data_ptr() - base.data_ptr()) // data.element_size() if rows * pitch else 0
    view = host[off: off + rows * pitch].reshape(rows, pitch)
    values = view[:, :n].copy()
    view[:, :n] = CANARY
    assert (host == CANARY).all(), f"{what}: written beyond the {n} values of a row"
    return values


def run_kernel(dev, case: hr.HeightsCase, storage: str, outside: str, zs_above_ground: bool = False) -> np.ndarray:
    """The kernel on the case in one storage shape: ``[n_pts, n_var, n_tgt]``.  Asserts that nothing is written outside a point's
    ``n_var x n_tgt`` rows (or a row's ``n_pts`` points) and that src, t, q, sp and zs are left as they were.  ``zs_above_ground``: hand
    the case's zs (with its NaN) to a call above the ground, which must not read it."""
    n_pts, n_var, n_lev, n_tgt = case.n_pts, case.n_var, case.n_lev, case.n_tgt
    columns = storage.startswith("columns")
    layout = COLUMNS if columns else FIELDS
    kinds = dict(src="columns-base+1", t="columns", q="columns-pitch+1", out="columns") if storage == MIXED else dict.fromkeys(("src", "t", "q", "out"), storage)
    rows = dict(src=n_var * n_lev, t=n_lev, q=n_lev, out=n_var * n_tgt)
    values = dict(src=case.x.reshape(n_pts, n_var * n_lev), t=case.per_point(case.geo.t), q=case.per_point(case.geo.q))
    stacks = {}
    for name in ("src", "t", "q", "out"):
        shape = (n_pts, rows[name]) if columns else (rows[name], n_pts)
        stacks[name] = allocate(*shape, kinds[name], case.T, dev, CANARY if name == "out" else float("nan"))
        if name != "out" and n_pts:
            if columns:
                stacks[name][:, : rows[name]] = torch.from_numpy(values[name]).to(dev)
            else:
                stacks[name][:, :n_pts] = torch.from_numpy(np.ascontiguousarray(values[name].T)).to(dev)
    sp = torch.from_numpy(case.per_point(case.geo.sp)).to(dev)
    zs = torch.from_numpy(case.per_point(case.zs)).to(dev) if case.reference == hr.SEA or zs_above_ground else None
    inputs = [("src", stacks["src"]), ("t", stacks["t"]), ("q", stacks["q"]), ("sp", sp)] + ([] if zs is None else [("zs", zs)])
    before = [x.clone() for _, x in inputs]
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    pitch = lambda name: stacks[name].shape[1]  # noqa: E731 - the view's row length IS its pitch (allocate); an empty view has no stride to ask
    native_heights.interpolate(stacks["src"], stacks["out"], stacks["t"], stacks["q"], sp, zs, f64(case.geo.A), f64(case.geo.B), f64(case.targets),
                               n_pts=n_pts, n_var=n_var, n_lev=n_lev, n_tgt=n_tgt, src_pitch=pitch("src"), t_pitch=pitch("t"), q_pitch=pitch("q"),
                               out_pitch=pitch("out"), layout=layout, reference=case.reference, outside=outside)
    torch.cuda.synchronize()
    bits = torch.int32 if case.T is np.float32 else torch.int64
    for (name, now), was in zip(inputs, before):
        assert torch.equal(now.view(bits), was.view(bits)), f"{case.name} {storage}: {name} was modified"
    what = f"{case.name} {storage} {outside}"
    if columns:
        return take(stacks["out"], n_var * n_tgt, what).reshape(n_pts, n_var, n_tgt)
    return np.ascontiguousarray(take(stacks["out"], n_pts, what).T).reshape(n_pts, n_var, n_tgt)


def every_storage(dev, case: hr.HeightsCase):
    """``compute(case, outside)`` for ``hr.check``: the first storage's result, after every other storage has given the same bytes (above
    the ground the first call is handed a zs it must not read, the others none)."""
    def compute(_, outside):
        first = run_kernel(dev, case, STORAGE[0], outside, zs_above_ground=True)
        for storage in STORAGE[1:]:
            assert run_kernel(dev, case, storage, outside).tobytes() == first.tobytes(), f"{case.name} {outside}: {storage} differs from {STORAGE[0]}"
        return first
    return compute


# ---- the kernel against the exact statement -----------------------------------------------------------------------------------------
REPORT: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        print("\nmodel levels to height levels, worst ulps of max(|x[a]|, |x[b]|) from exact (kernel / numpy's float64 / bound):")
        for key, row in sorted(REPORT.items()):
            print(f"  {key:<60} kernel {row['kernel']:11.4f}   numpy {row['numpy_float64']:11.4f}   bound {row['bound']:.8g}")
        if os.environ.get("ATX_HEIGHTS_ULPS_JSON"):
            with open(os.environ["ATX_HEIGHTS_ULPS_JSON"], "w") as f:
                json.dump(dict(unit="ulps of max(|x[a]|, |x[b]|) in the stack's type", kernel=REPORT), f, indent=1)
                f.write("\n")


@pytest.mark.parametrize("shape", hr.SHAPES, ids=lambda s: "-".join(str(v) for v in s))
@pytest.mark.parametrize("T", WIDTHS)
def test_the_kernel_is_within_its_budget_of_the_exact_statement(dev, T, shape):
    """Every storage shape and both policies through the one comparison the host test plants defects in."""
    case = hr.make_case(T, *shape)
    report: dict = {}
    hr.check(every_storage(dev, case), [case], NUMPY_WORST_HEIGHTS, report)
    REPORT.update(report)


@pytest.mark.parametrize("reference", [hr.GROUND, hr.SEA])
@pytest.mark.parametrize("T", WIDTHS)
def test_one_level_of_a_one_level_model_is_the_restatement_bit_for_bit(dev, T, reference):
    """n_lev = 1 with n_half = 2: alpha = ln 2, no logarithm and no interior — every result is a copy or NaN."""
    case = hr.make_case(T, 65, 1, hr.WHOLE, 13, 2, reference)
    assert case.geo.n_half == 2
    for outside in (hr.NEAREST, hr.MISSING):
        got = every_storage(dev, case)(case, outside)
        want = hr.reference(case, outside)
        hr.assert_same_bits(got, want, f"{case.name} {outside}")
        assert np.isnan(got[4]).all() and np.isnan(case.geo.sp[4])  # a NaN sp reaches no c here, and still the result is NaN


@pytest.mark.parametrize("T", WIDTHS)
def test_a_column_that_is_not_monotone_is_counted_whole(dev, T):
    """A few negative t bend c: the bisection does not apply, the whole-column count runs.  NaN where the restatement has them and the
    copies bit for bit in both widths; float64 within the rule with numpy's worst measured ON THIS CASE (here, on the CPU); float32's rule
    needs w inside [0, 1], which a bent column does not give."""
    case = hr.bent_case(T)
    hr.check(every_storage(dev, case), [case], hr.numpy_worst, accuracy=T is np.float64)


def test_interpolating_the_geopotential_itself_returns_the_target(dev):
    """float64, above the sea, x = what ``atx_geopotential_on_model_levels`` stores for the same inputs: c's own bits.  Then every interior
    result is its target G up to the roundings of w and y.  With u = 2^-53, N = c[a] - G in [0, D), D = c[a] - c[b] > 0 and
    M = max(|c[a]|, |c[b]|): fl(N) = N (1 + e1), fl(D) = D (1 + e2), w = fl(N) / fl(D) (1 + e3), fl(c[b] - c[a]) = -D (1 + e4),
    s = w fl(c[b] - c[a]) (1 + e5) = -N (1 + theta) with |theta| <= 5 u + O(u^2), y = (c[a] + s) (1 + e6) = (G - N theta) (1 + e6), so
    |y - G| <= u |G| + 5 u N + O(u^2) <= 11 u M + O(u^2), because |G| <= M and N < D <= 2 M; and u M < one ulp of M.  The bound: 12 ulps of M."""
    case = hr.make_case(np.float64, 257, 60, hr.WHOLE, 13, 1, hr.SEA, False)
    smallest, disagreements = hr.margins(case)
    assert smallest >= hr.MARGIN and disagreements == 0  # the kernel's brackets are numpy's
    n_pts, n_lev = case.n_pts, case.n_lev
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    t, q, sp, zs = (up(case.per_point(a)) for a in (case.geo.t, case.geo.q, case.geo.sp, case.zs))
    A, B = up(case.geo.A), up(case.geo.B)
    z = torch.empty_like(t)
    native_geopotential.geopotential(t, q, sp, zs, A, B, z, n_pts=n_pts, n_lev=n_lev, t_pitch=n_lev, q_pitch=n_lev, out_pitch=n_lev, layout=COLUMNS)
    out = torch.empty((n_pts, case.n_tgt), dtype=torch.float64, device=dev)
    native_heights.interpolate(z, out, t, q, sp, zs, A, B, up(case.targets), n_pts=n_pts, n_var=1, n_lev=n_lev, n_tgt=case.n_tgt, src_pitch=n_lev,
                               t_pitch=n_lev, q_pitch=n_lev, out_pitch=case.n_tgt, layout=COLUMNS, reference="sea", outside="missing")
    torch.cuda.synchronize()
    y, c = out.cpu().numpy(), z.cpu().numpy()
    found = hr.brackets(case)
    checked, worst = 0, 0.0
    for p in range(n_pts):
        for i, (kind, a, b, _) in enumerate(found[p % case.n_columns]):
            if kind != hr.INTERIOR:
                continue
            M = max(abs(c[p, a]), abs(c[p, b]))
            apart = abs(y[p, i] - case.targets[i]) / np.spacing(M)
            worst, checked = max(worst, apart), checked + 1
            assert apart <= 12.0, (p, i, a, b, apart)
    print(f"interpolating c itself: {checked} interior results, at most {worst:.2f} ulps of max(|c[a]|, |c[b]|) from their target")
    assert checked > 1000


# ---- the layer below the filter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [COLUMNS, FIELDS], ids=["columns", "fields"])
def test_interpolate_to_heights_takes_three_stacks(dev, layout):
    case = hr.make_case(np.float32, 65, 17, hr.SUBSET, 13, 2, hr.SEA)
    pinned = hr.numpy_worst(hr.make_case(np.float64, 65, 17, hr.SUBSET, 13, 2, hr.SEA))  # of the float64 case of the shape, on the CPU
    x = Stack.from_fields(list(case.x.reshape(case.n_pts, -1).T), dev=dev, layout=layout)
    t = Stack.from_fields(list(case.per_point(case.geo.t).T), dev=dev, layout=layout)
    q = Stack.from_fields(list(case.per_point(case.geo.q).T), dev=dev, layout=layout)
    sp, zs = torch.from_numpy(case.per_point(case.geo.sp)).to(dev), torch.from_numpy(case.per_point(case.zs)).to(dev)

    def compute(_, outside):
        out = interpolate_to_heights(x, t, q, sp, zs, case.geo.A, case.geo.B, case.heights_m, n_var=2, reference="sea", outside=outside)
        assert (out.n_pts, out.n_lev, out.layout, out.dtype) == (case.n_pts, 2 * case.n_tgt, layout, torch.float32)
        return np.ascontiguousarray(out.numpy().T).reshape(case.n_pts, 2, case.n_tgt)

    hr.check(compute, [case], lambda c: pinned)


# ---- the filter, end to end --------------------------------------------------------------------------------------------------------------
N_LEV = 17
LEVELS = [10, 100, 250.5, 3000]  # metres
DATES = (20260101, 20260102)
PARAMS = ("u", "v", "t")


def small_world(dtype=np.float64, lnsp=False):
    grid = lookup([10.0, 10.0])  # 684 points: more than one workgroup in either layout, and few enough for the exact evaluator
    lat, lon = np.asarray(grid["latitudes"], dtype=np.float64), np.asarray(grid["longitudes"], dtype=np.float64)
    n = len(lat)
    rng = np.random.default_rng(29)
    A, B = gr.eta_table(N_LEV + 1)
    specs, cases = [], {}
    for date in DATES:
        common = dict(latitudes=lat, longitudes=lon, date=date, time=0, step=0)
        sp = rng.uniform(50000.0, 105000.0, n).astype(dtype)
        zs = rng.uniform(-500.0, 30000.0, n).astype(dtype)
        columns = dict(t=(250.0 + 30.0 * rng.standard_normal((n, N_LEV))).astype(dtype), q=rng.uniform(0.0, 0.02, (n, N_LEV)).astype(dtype),
                       u=(20.0 * rng.standard_normal((n, N_LEV))).astype(dtype), v=(20.0 * rng.standard_normal((n, N_LEV))).astype(dtype))
        specs.append(dict(values=(280.0 + rng.standard_normal(n)).astype(dtype), param="2t", levtype="sfc", **common))
        specs.append(dict(values=zs, param="z", levtype="ml", levelist=1, **common))  # as MARS keeps it
        for level in rng.permutation(N_LEV) + 1:  # the levels in no order
            for param in ("v", "t", "q", "u"):
                specs.append(dict(values=columns[param][:, level - 1].copy(), param=param, levtype="ml", levelist=int(level), **common))
        if lnsp:
            specs.append(dict(values=np.log(sp.astype(np.float64)).astype(dtype), param="lnsp", levtype="ml", levelist=1, **common))
        else:
            specs.append(dict(values=sp, param="sp", levtype="sfc", **common))
        geo = gr.GeoCase(f"hl-world-{date}-{np.dtype(dtype).name}", dtype, A, B, sp, zs, columns["t"], columns["q"])
        cases[date] = (geo, zs, columns)
    return fieldlist_from_dicts(specs, mars=True), cases, dict(A=A.tolist(), B=B.tolist())


def world_case(cases, date, params, reference, dtype) -> hr.HeightsCase:
    geo, zs, columns = cases[date]
    x = np.ascontiguousarray(np.stack([columns[p] for p in params], axis=1))
    return hr.HeightsCase(f"{geo.name}-{reference}-{'-'.join(params)}", dtype, geo, zs, x, np.array(LEVELS, dtype=np.float64), reference)


def assert_under_the_rule(got: np.ndarray, case: hr.HeightsCase) -> None:
    """``got`` under "nearest": the rule with numpy's worst ON THIS CASE (measured here, on the CPU); the copies bit for bit."""
    want = hr.reference(case)
    value, unit = hr.exact_reference(case)
    interior = np.vectorize(lambda v: v is not None, otypes=[bool])(value)
    assert interior.any() and not interior.all()
    hr.assert_same_bits(np.where(interior, 0, got).astype(got.dtype), np.where(interior, 0, want).astype(got.dtype), case.name + " (copies)")
    e = hr.errors(got, value, unit)
    limit = hr.bound(case, hr.numpy_worst(case))
    assert np.nanmax(e) <= limit, f"{case.name}: {np.nanmax(e):.4f} ulps from exact > {limit:.6g}"


@pytest.mark.parametrize("reference", [hr.GROUND, hr.SEA])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_filter_end_to_end(dev, monkeypatch, dtype, reference):
    data, cases, AB = small_world(dtype)
    # above the ground the surface z (z, ml, 1) would be a variable with one level: params names what is wanted; above the sea it is zs
    params = PARAMS if reference == hr.GROUND else ("v", "t", "q", "u")  # (the default: every ml param, in first-seen order)
    f = create_filter_by_name("ml_to_hl", levels=LEVELS, model_level_AB=AB, reference=reference, params=list(PARAMS) if reference == hr.GROUND else None)
    launches = []
    real = native_heights.interpolate
    monkeypatch.setattr(native_heights, "interpolate", lambda *a, **k: (launches.append((k["n_var"], k["n_lev"], k["n_tgt"])), real(*a, **k))[1])
    result = list(f.forward(data))
    assert launches == [(len(params), N_LEV, len(LEVELS))] * len(DATES)  # ONE launch per group
    kept = list(data)
    assert all(a is b for a, b in zip(result, kept)) and len(result) == len(kept) + len(DATES) * len(params) * len(LEVELS)  # every input passes through
    new = result[len(kept):]
    order = [p for p in ("v", "t", "q", "u") if p in params]  # first seen first
    assert [(g.metadata("date"), g.metadata("param"), g.metadata("levtype"), g.metadata("levelist")) for g in new] == [
        (date, param, "hl", level) for date in DATES for param in order for level in LEVELS]
    assert [type(g.metadata("levelist")) for g in new[: len(LEVELS)]] == [int, int, float, int]
    assert len({id(g.stack_ref()[0]) for g in new}) == len(DATES) and all(g.stack_ref()[0].data.is_cuda for g in new)  # levels of one resident stack
    assert all(g.stack_ref()[0].dtype == (torch.float32 if dtype is np.float32 else torch.float64) for g in new)
    assert new[0].metadata(namespace="mars")["levtype"] == "hl" and new[0].metadata(namespace="mars")["levelist"] == 10
    per_date = len(order) * len(LEVELS)
    for i, date in enumerate(DATES):
        got = np.stack([g.to_numpy(flatten=True) for g in new[i * per_date:(i + 1) * per_date]], axis=1).reshape(-1, len(order), len(LEVELS))
        assert got.dtype == dtype
        assert_under_the_rule(got, world_case(cases, date, order, reference, dtype))


def test_one_float64_field_makes_the_group_float64(dev):
    data, cases, AB = small_world(np.float32)
    fields = list(data)
    i = next(i for i, g in enumerate(fields) if g.metadata("param") == "sp" and g.metadata("date") == DATES[0])
    fields[i] = fields[i].clone(values=fields[i].to_numpy(flatten=True).astype(np.float64))
    new = [g for g in create_filter_by_name("ml_to_hl", levels=LEVELS, model_level_AB=AB, params=["u"]).forward(FieldList(fields)) if g.metadata("levtype") == "hl"]
    assert [g.stack_ref()[0].dtype for g in new[: len(LEVELS)]] == [torch.float64] * len(LEVELS)
    assert [g.stack_ref()[0].dtype for g in new[len(LEVELS):]] == [torch.float32] * len(LEVELS)


def test_fields_given_in_the_fields_layout_give_the_same_bits(dev):
    data, cases, AB = small_world(np.float64)
    f = create_filter_by_name("ml_to_hl", levels=LEVELS, model_level_AB=AB, reference="sea", outside="missing")
    host = list(data)
    stack = Stack.from_fields([g.to_numpy(flatten=True) for g in host], dev=dev, layout=FIELDS)
    resident = FieldList([new_field_from_stack(stack, i, template=g) for i, g in enumerate(host)])
    a = [g for g in f.forward(data) if g.metadata("levtype") == "hl"]
    b = [g for g in f.forward(resident) if g.metadata("levtype") == "hl"]
    assert len(a) == len(b) == len(DATES) * 4 * len(LEVELS)
    assert all(g.stack_ref()[0].layout == COLUMNS for g in a) and all(g.stack_ref()[0].layout == FIELDS for g in b)
    for x, y in zip(a, b):
        assert (x.metadata("date"), x.metadata("param"), x.metadata("levelist")) == (y.metadata("date"), y.metadata("param"), y.metadata("levelist"))
        assert x.to_numpy(flatten=True).tobytes() == y.to_numpy(flatten=True).tobytes(), "FIELDS against COLUMNS"


def test_lnsp_to_sp_then_ml_to_hl_runs(dev):
    data, cases, AB = small_world(np.float64, lnsp=True)
    hl = create_filter_by_name("ml_to_hl", levels=LEVELS, model_level_AB=AB, params=["u", "v"])
    with pytest.raises(ValueError, match=r"lnsp_to_sp \| ml_to_hl"):
        hl.forward(data)
    got = [g for g in (create_filter_by_name("lnsp_to_sp") | hl).forward(data) if g.metadata("levtype") == "hl"]
    assert [(g.metadata("date"), g.metadata("param"), g.metadata("levelist")) for g in got] == [(d, p, v) for d in DATES for p in ("v", "u") for v in LEVELS]
    assert all(g.stack_ref() is not None and g.stack_ref()[0].data.is_cuda and np.isfinite(g.to_numpy(flatten=True)).all() for g in got)
