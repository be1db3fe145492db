"""``sort_by``, ``drop_duplicates`` and ``drop`` on the device: the three kernels of ``csrc/atx_obs_rowset.hip`` through ``native``
directly — at wave and workgroup edges and past the grid cap, where a lane takes a second row — against the numpy restatement
(tests/rowset_restatement.py), and the filters against the frames the reference's own ``forward`` returned
(tests/golden/rowset.json) on a DataFrame, a dict of arrays and a dict of device tensors.  Every comparison is exact: the feature has
no tolerance.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import rowset_restatement as R
from anemoi_transform_amd import native, obs
from anemoi_transform_amd.filters import create_filter_by_name

pytestmark = pytest.mark.gpu

PAST_CAP = R.GRID_CAP_ROWS + 300
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, PAST_CAP)
GOLDEN = R.load_golden()
TAKE_DTYPES = (np.float64, np.uint8, np.int16, np.float32, np.int64, np.bool_, np.int32, np.float16, np.int8)  # widths 8 1 2 4 8 1 4 2 1


def _up(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- atx_obs_order_key -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", list(R.CODES))
def test_order_key_equals_the_restatement_for_every_dtype(dev, code):
    specials = R.key_specials(code)
    if code.startswith("float"):  # subnormals and infinities of both signs are among them
        tiny = np.finfo(specials.dtype).tiny
        assert ((np.abs(specials) > 0) & (np.abs(specials) < tiny)).any() and {np.inf, -np.inf} <= set(specials[np.isinf(specials)].tolist())
        assert np.isnan(specials).sum() >= 4 and (np.signbit(specials) & (specials == 0)).any()
    for n in SIZES:
        x = np.resize(specials, n)
        want = R.order_key(x, datetime=code == "datetime")
        key = torch.full((n,), -7, dtype=torch.int64, device=dev)
        native.obs_order_key(_up(x, dev), key, R.CODES[code])
        assert np.array_equal(key.cpu().numpy(), want), (code, n)
        if code != "datetime":  # the default code is the dtype's; obs.order_keys takes the same route from a host array
            assert np.array_equal(obs.order_keys(x, dev).cpu().numpy(), want), (code, n)
    dates = R.DATE_POOL
    assert np.array_equal(obs.order_keys(dates, dev).cpu().numpy(), R.order_key(dates))
    assert np.array_equal(obs.order_keys(_up(dates.view(np.int64), dev), datetime=True).cpu().numpy(), R.order_key(dates))


def test_order_keys_widens_narrow_columns_exactly_and_ranks_strings(dev):
    half = np.array([0.0, -0.0, np.nan, 65504.0, -65504.0, 6e-8, np.inf], dtype=np.float16)
    assert np.array_equal(obs.order_keys(half, dev).cpu().numpy(), R.order_key(half.astype(np.float64)))
    wide = np.array([0, 65535, 7], dtype=np.uint16)
    assert obs.order_keys(wide, dev).cpu().tolist() == [0, 65535, 7]
    assert obs.order_keys(np.array([0, 2**32 - 1], dtype=np.uint32), dev).cpu().tolist() == [0, 2**32 - 1]
    names = np.array(R.NAME_POOL, dtype=object)
    assert obs.order_keys(names, dev).cpu().tolist() == R.string_ranks(names).tolist()
    with pytest.raises(ValueError, match="uint64"):
        obs.order_keys(torch.zeros(4, dtype=torch.uint64, device=dev))


# ---- atx_obs_mark_first ------------------------------------------------------------------------------------------------------------------------
def _mark(keys, order, dev, prefill=0):
    keep = torch.full((order.size,), prefill, dtype=torch.uint8, device=dev)
    d_keys, d_order = [_up(k, dev) for k in keys], _up(order, dev)
    for j in range(0, len(keys), native.MAX_ROWSET_COLUMNS):
        native.obs_mark_first(d_keys[j:j + native.MAX_ROWSET_COLUMNS], d_order, keep, accumulate=j > 0)
    return keep.cpu().numpy()


@pytest.mark.parametrize("n_keys", [1, 16, 17])
def test_mark_first_equals_the_restatement(dev, n_keys):
    rng = np.random.default_rng(100 + n_keys)
    for n in SIZES:
        keys = [rng.integers(0, 2 if n_keys > 1 else 9, n) for _ in range(n_keys)]
        # the kernel's statement holds for ANY permutation: a random one at every size, and the sorted one where it is cheap
        orders = [rng.permutation(n).astype(np.int64)] + ([R.stable_order(keys)] if n and n <= 4096 else [])
        for order in orders:
            got = _mark(keys, order, dev, prefill=9)  # a plain launch writes every byte, 0 or 1
            assert np.array_equal(got, R.mark_first(keys, order)), (n_keys, n)
        if n and n <= 4096:
            assert np.array_equal(np.nonzero(got)[0], R.first_occurrences(keys))


@pytest.mark.parametrize("which", ["last", "first"])
def test_mark_first_sees_a_difference_in_one_key_only(dev, which):
    """Seventeen keys of which sixteen are constant: the one that differs is the last (it arrives with the accumulating launch) or the
    first (the accumulating launch adds nothing and must clear nothing)."""
    n = 257
    rng = np.random.default_rng(5)
    varying = rng.integers(0, 5, n)
    keys = [np.full(n, 3, dtype=np.int64) for _ in range(17)]
    keys[16 if which == "last" else 0] = varying
    order = R.stable_order(keys)
    got = _mark(keys, order, dev)
    assert np.array_equal(got, R.mark_first(keys, order)) and got.sum() == 5
    assert np.array_equal(np.nonzero(got)[0], R.first_occurrences([varying]))
    # accumulate never clears: a second, accumulating launch over constant keys leaves every mark
    keep = _up(got, dev)
    native.obs_mark_first([_up(keys[1], dev)], _up(order, dev), keep, accumulate=True)
    again = keep.cpu().numpy()
    assert np.array_equal(again, got) and again[order[0]] == 1


# ---- atx_obs_take_rows -------------------------------------------------------------------------------------------------------------------------
def _columns(n: int, n_cols: int, rng) -> list[np.ndarray]:
    out = []
    for c in range(n_cols):
        dtype = np.dtype(TAKE_DTYPES[c % len(TAKE_DTYPES)])
        out.append(rng.integers(0, 256, n * dtype.itemsize, dtype=np.uint8).view(dtype) if dtype != np.bool_ else rng.random(n) < 0.5)
    return out


def _index_patterns(n: int, rng) -> dict[str, np.ndarray]:
    patterns = {"identity": np.arange(n, dtype=np.int64), "reversed": np.arange(n, dtype=np.int64)[::-1].copy(),
                "random": rng.permutation(n).astype(np.int64)}
    if n:
        patterns["repeated"] = rng.integers(0, n, n + 7).astype(np.int64)  # more rows out than in, rows taken several times
    return patterns


@pytest.mark.parametrize("n_cols", [1, 16, 17])
def test_take_rows_equals_numpy_indexing(dev, n_cols):
    rng = np.random.default_rng(200 + n_cols)
    for n in SIZES:
        if n == PAST_CAP and n_cols == 16:
            continue  # the cap is crossed with one column and with seventeen
        columns = _columns(n, n_cols, rng)
        table = {f"c{c}": col for c, col in enumerate(columns)}
        resident = {name: _up(col, dev) for name, col in table.items()}
        for name, rows in _index_patterns(n, rng).items():
            if n == PAST_CAP and name not in ("random", "repeated"):
                continue
            got = obs.take_rows(resident if name != "identity" else table, _up(rows, dev) if name != "reversed" else rows)
            assert list(got) == list(table)
            for key, col in table.items():
                assert got[key].is_cuda and R.same_bits(got[key].cpu().numpy(), col[rows]), (n_cols, n, name, key)
    assert obs.take_rows({}, np.arange(3)) == {}


def test_take_rows_keeps_dates_as_nanoseconds_and_refuses_what_cannot_live_on_the_device(dev):
    dates = R.DATE_POOL
    got = obs.take_rows({"date": dates, "flag": np.array([True, False] * 4)}, np.array([7, 0, 0, 3]), dev=dev)
    assert got["date"].dtype == torch.int64 and got["date"].cpu().tolist() == dates.view(np.int64)[[7, 0, 0, 3]].tolist()
    assert got["flag"].dtype == torch.bool and got["flag"].cpu().tolist() == [False, True, True, False]
    with pytest.raises(ValueError, match="cannot live on the device"):
        obs.take_rows({"name": np.array(["a", "b"], dtype=object)}, np.array([0]), dev=dev)
    with pytest.raises(ValueError, match="16 bytes"):
        obs.take_rows({"z": np.zeros(2, dtype=np.complex128)}, np.array([0]), dev=dev)
    with pytest.raises(ValueError, match="differ in length"):
        obs.take_rows({"a": np.zeros(2), "b": np.zeros(3)}, np.array([0]), dev=dev)


@pytest.mark.parametrize("n", [65, PAST_CAP])
def test_take_rows_counts_rows_outside_the_table_and_leaves_them_untouched(dev, n):
    rng = np.random.default_rng(300 + n)
    columns = _columns(n, 17, rng)
    rows = rng.integers(0, n, n).astype(np.int64)
    bad_at = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 5)]))
    rows[bad_at] = np.resize(np.array([-1, n, R.I64_MIN, R.I64_MAX, n + 2**31, -n - 1], dtype=np.int64), bad_at.size)
    good = np.ones(n, dtype=bool)
    good[bad_at] = False
    d_cols, d_rows = [_up(c, dev) for c in columns], _up(rows, dev)
    outs = [torch.full((n * c.dtype.itemsize,), 0xA5, dtype=torch.uint8, device=dev).view(d.dtype) for c, d in zip(columns, d_cols)]
    n_bad = torch.full((2,), -1, dtype=torch.int64, device=dev)
    native.obs_take_rows(d_cols[:16], outs[:16], d_rows, n_bad[0:1])
    native.obs_take_rows(d_cols[16:], outs[16:], d_rows, n_bad[1:2])
    assert n_bad.cpu().tolist() == [bad_at.size, bad_at.size]
    for col, out in zip(columns, outs):
        got = out.cpu().numpy()
        assert R.same_bits(got[good], col[rows[good]])
        assert (got[~good].view(np.uint8) == 0xA5).all()  # nothing written for a row outside the table
    with pytest.raises(IndexError, match=f"{bad_at.size} of {n} row indices"):
        obs.take_rows({f"c{c}": col for c, col in enumerate(d_cols)}, d_rows)
    native.obs_take_rows(d_cols[:1], outs[:1], _up(np.arange(n, dtype=np.int64), dev), n_bad[0:1])  # the counter is set, not added to
    assert int(n_bad[0]) == 0


# ---- sort_order / first_rows ---------------------------------------------------------------------------------------------------------------------
def test_sort_order_and_first_rows_past_the_cap(dev):
    """Three keys — float64 with zeros of both signs and NaNs, int64 beyond 2^53, bool — over more rows than the grid holds lanes."""
    rng = np.random.default_rng(77)
    n = PAST_CAP
    columns = [R.F64_POOL[rng.integers(0, R.F64_POOL.size, n)], R.I64_POOL[rng.integers(0, R.I64_POOL.size, n)], rng.random(n) < 0.5]
    keys = [R.order_key(c) for c in columns]
    order = obs.sort_order([_up(c, dev) for c in columns])
    assert order.dtype == torch.int64 and np.array_equal(order.cpu().numpy(), R.stable_order(keys))
    first = obs.first_rows(columns, dev)
    assert np.array_equal(first.cpu().numpy(), R.first_occurrences(keys)) and first.numel() == 15 * 10 * 2
    assert obs.first_rows([np.zeros(0)], dev).numel() == 0 and obs.sort_order([np.zeros(0)], dev).numel() == 0


# ---- the filters against the recorded frames --------------------------------------------------------------------------------------------------
def _as_resident(table: dict, dev) -> dict:
    """Numeric columns as device tensors (dates as int64 nanoseconds); a string column cannot live there and stays a host array."""
    out = {}
    for name, col in table.items():
        if col.dtype.kind == "O":
            out[name] = col
        else:
            out[name] = _up(col.view(np.int64) if col.dtype.kind == "M" else col, dev)
    return out


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["id"] for c in GOLDEN["cases"]])
def test_filters_equal_the_recorded_frames_on_three_kinds_of_table(dev, case):
    pd = pytest.importorskip("pandas")
    stored = GOLDEN["tables"][case["table"]]
    table = {c: stored["columns"][c] for c in case["columns"]}
    f = create_filter_by_name(case["filter"], **case["config"])

    frame = pd.DataFrame(table, index=stored["index"])
    before = frame.copy(deep=True)
    got = f(frame)
    want = pd.DataFrame(case["expected"], index=case["index"])
    pd.testing.assert_frame_equal(got, want, check_exact=True)  # values, dtypes, column order and the index labels
    assert all(R.same_bits(got[c].to_numpy(), case["expected"][c]) for c in want.columns)  # a NaN's payload, a zero's sign
    assert frame.equals(before) and got is not frame
    if "literals" in case:  # R: tests/tabular_filters/test_sort_by.py:41-49
        assert got.reset_index(drop=True).equals(pd.DataFrame({c: np.array(v) for c, v in case["literals"].items()}))
    if "dropped_index" in case:  # R: tests/tabular_filters/test_drop_duplicates.py:38, :77, :95
        assert got.equals(frame.drop(index=case["dropped_index"]))

    arrays = dict(table)
    got = f(arrays)
    assert got is not arrays and list(got) == list(case["expected"]) and list(arrays) == case["columns"]
    for name, column in case["expected"].items():
        assert isinstance(got[name], np.ndarray) and R.same_bits(got[name], column), (case["id"], name)

    resident = _as_resident(table, dev)
    got = f(resident)
    assert got is not resident and list(got) == list(case["expected"]) and list(resident) == case["columns"]
    for name, column in case["expected"].items():
        if column.dtype.kind == "O":
            assert R.same_bits(got[name], column)
            continue
        assert isinstance(got[name], torch.Tensor) and got[name].is_cuda and got[name].dtype == resident[name].dtype, (case["id"], name)
        want_bits = column.view(np.int64) if column.dtype.kind == "M" else column
        assert R.same_bits(got[name].cpu().numpy(), want_bits), (case["id"], name)
        if case["filter"] == "drop":
            assert got[name] is resident[name]  # nothing is copied


def test_a_chain_of_device_tensors_stays_on_the_device_and_equals_pandas(dev):
    """``drop_duplicates | sort_by | drop | add_healpix`` on a dict of device tensors against the same chain step by step through
    pandas (``drop_duplicates``, ``sort_values(kind="stable")``, ``drop``) and the existing ``add_healpix`` filter on the DataFrame."""
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(99)
    n = 700
    place = rng.integers(0, 60, n)
    lat_pool, lon_pool = rng.uniform(-89.0, 89.0, 60), rng.uniform(-180.0, 359.0, 60)
    table = {
        "date": R.DATE_POOL[rng.integers(0, R.DATE_POOL.size, n)],
        "station": R.I64_POOL[rng.integers(0, R.I64_POOL.size, n)],
        "latitude": lat_pool[place],
        "longitude": lon_pool[place],
        "obsvalue": np.where(rng.random(n) < 0.1, np.nan, rng.normal(280.0, 30.0, n)),
        "scratch": rng.integers(-100, 100, n).astype(np.int32),
        "flag": rng.random(n) < 0.5,
    }
    chain = [create_filter_by_name("drop_duplicates", columns=["date", "station", "latitude"]),
             create_filter_by_name("sort_by", columns=["date", "latitude", "station"]),
             create_filter_by_name("drop", columns=["scratch"]),
             create_filter_by_name("add_healpix", nside=16)]
    got = _as_resident(table, dev)
    for f in chain:
        got = f(got)
        assert all(isinstance(col, torch.Tensor) and col.is_cuda for col in got.values()), repr(f)

    frame = pd.DataFrame(table)
    frame = frame.drop_duplicates(subset=["date", "station", "latitude"])
    frame = frame.sort_values(by=["date", "latitude", "station"], kind="stable")
    frame = frame.drop(labels=["scratch"], axis=1)
    frame = chain[3](frame)
    assert list(got) == list(frame.columns) and 100 < len(frame) < n
    for name in frame.columns:
        want = frame[name].to_numpy()
        want = want.view(np.int64) if want.dtype.kind == "M" else want
        assert R.same_bits(got[name].cpu().numpy(), want), name


@pytest.mark.parametrize("n", [1, 257])
def test_table_take_gathers_what_can_live_on_the_device_and_indexes_the_rest_on_the_host(dev, monkeypatch, n):
    """``Table.take`` on a resident mapping of 18 numeric columns and one of strings: the numeric ones come back as device tensors from
    two launches, the strings as a numpy array, all of it numpy's indexing — for rows with repeats and for descending rows."""
    from anemoi_transform_amd.tables import Table

    rng = np.random.default_rng(400 + n)
    host = {f"c{c}": col for c, col in enumerate(_columns(n, 18, rng))}
    host = {**dict(list(host.items())[:5]), "name": np.array(R.NAME_POOL, dtype=object)[rng.integers(0, len(R.NAME_POOL), n)], **dict(list(host.items())[5:])}
    resident = _as_resident(host, dev)
    calls = []
    real = native.obs_take_rows
    monkeypatch.setattr(native, "obs_take_rows", lambda cols, outs, rows, n_bad: (calls.append(len(cols)), real(cols, outs, rows, n_bad))[1])
    for rows in (rng.integers(0, n, n + 7).astype(np.int64), np.arange(n, dtype=np.int64)[::-1].copy()):
        del calls[:]
        got = Table(resident).take(_up(rows, dev))
        assert calls == [16, 2] and got is not resident and list(got) == list(host) and list(resident) == list(host)
        assert isinstance(got["name"], np.ndarray) and R.same_bits(got["name"], host["name"][rows])
        for name, col in host.items():
            if name != "name":
                assert got[name].is_cuda and got[name].dtype == resident[name].dtype and R.same_bits(got[name].cpu().numpy(), col[rows]), (n, name)
    del calls[:]
    part = Table(resident).take(_up(rows, dev), names=["name", "c17", "c0"])
    assert calls == [2] and list(part) == ["name", "c17", "c0"] and R.same_bits(part["c17"].cpu().numpy(), host["c17"][rows])
