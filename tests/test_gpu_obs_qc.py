"""The row-program kernel (csrc/atx_obs_row_program.hip) and the nine tabular QC filters on the device.

- ``native.obs_column_ops`` with codes of the second family against the plain numpy interpreter (tests/row_program_restatement.py), bit for
  bit: every code, operands from registers and from memory, intermediates without an output, outputs in place, a SCALAR tensor of one
  element, n = 0, 1, 63, 64, 65, 257, 4099 (one lane, the edges of a wave, more than one workgroup), guard elements before and after
  every row.
- Every filter against the frames the reference itself returned (tests/golden/obs_qc.json): values to the bit, dtypes, column order,
  index labels — on a DataFrame, a dict of arrays and a dict of device tensors, which comes back as device tensors on the same device,
  the caller's tensors unchanged.
- A resident chain through the new filters, and the four dispatchers.
Everything is exact: there is no tolerance in this file.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import row_program_restatement as R
from anemoi_transform_amd import native, obs
from anemoi_transform_amd.filters import create_filter_by_name

pytestmark = pytest.mark.gpu
GOLDEN = R.load_golden()
SIZES = (0, 1, 63, 64, 65, 257, 4099)
SENTINEL = -12345.678
PAYLOAD_NAN = np.array([0x7FF4000000ABCDEF, 0xFFF8000000000001], dtype=np.uint64).view(np.float64)  # a signalling and a negative quiet NaN

# (operation, src, input, output): input "x" / "w" / "v" a row, "s0" / "s1" a scalar; output "new", "same" (in place) or None
PROGRAMS = {
    "compares": [("copy", -1, "x", "new"), ("scalar", -1, "s0", None), ("cmp_gt", 0, None, "new"), ("is_nan", -1, "w", "new"),
                 ("cmp_lt", -1, "x", None), ("not", 4, None, "new"), ("cmp_eq", -1, "w", "new"), ("scalar", -1, "s1", "new"),
                 ("cmp_ne", 0, None, "new"), ("copy", -1, "w", None), ("cmp_ge", 0, None, "new"), ("scalar", -1, "s0", None),
                 ("cmp_le", -1, "w", "new"), ("scalar", -1, "s1", None), ("abs_gt", -1, "x", "new"), ("and", 2, None, "new")],
    "selects": [("is_nan", -1, "x", None), ("or", -1, "w", "new"), ("nan_where", -1, "x", "new"), ("scalar", -1, "s0", None),
                ("clip_low", -1, "x", None), ("scalar", -1, "s1", None), ("clip_high", 4, None, "new"), ("scalar", -1, "s0", None),
                ("fill_nan", -1, "w", "same"), ("copy", 8, None, "new"), ("nan_where", -1, "v", "same"), ("not", 10, None, "new"),
                ("or", 1, None, "new")],
    "compares_with_a_row": [("copy", -1, "w", None), ("cmp_ge", -1, "x", "new"), ("copy", -1, "w", None), ("cmp_eq", -1, "x", "new"),
                            ("copy", -1, "w", None), ("cmp_ne", -1, "x", "new"), ("copy", -1, "w", None), ("clip_low", -1, "x", "new"),
                            ("copy", -1, "w", None), ("clip_high", -1, "x", "new"), ("copy", -1, "w", None), ("fill_nan", -1, "x", "new"),
                            ("copy", -1, "w", None), ("abs_gt", -1, "x", "new"), ("and", -1, "x", "new"), ("or", 14, None, "new")],
    "one_copy": [("copy", -1, "x", "new")],
    "one_scalar": [("scalar", -1, "s1", "new")],
    "copy_in_place": [("copy", -1, "x", "same"), ("is_nan", 0, None, "new")],
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    d = torch.device("cuda", 0)
    torch.cuda.set_device(d)
    native.load()
    return d


def _rows(n: int) -> dict:
    """Three rows of n values: the specials (payload NaNs, both zeros, infinities, values on and beside the scalars) first, random beyond."""
    rng = np.random.default_rng(4200 + n)
    pool = np.concatenate([PAYLOAD_NAN, R.value_pool()])
    out = {}
    for name in ("x", "w", "v"):
        a = np.where(rng.random(n) < 0.4, rng.choice(pool, n), np.round(rng.standard_normal(n) * 3.0, 1))
        a[:min(n, len(pool))] = rng.permutation(pool)[:n]
        out[name] = a
    return out


def _guarded(n: int, values=None, dev=None):
    whole = torch.full((n + 128,), SENTINEL, dtype=torch.float64, device=dev)
    row = whole[32:32 + n]
    if values is not None:
        row.copy_(torch.from_numpy(values.view(np.int64).copy()).view(torch.float64))  # the bits, whatever the copy does with a signalling NaN
    return whole, row


def _guards_hold(whole: torch.Tensor, n: int) -> bool:
    return bool((whole[:32] == SENTINEL).all()) and bool((whole[32 + n:] == SENTINEL).all())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_kernel_against_the_interpreter(dev, name, n):
    host = _rows(n)
    scalars = {"s0": np.array([2.5]), "s1": np.array([0.1])}
    device = {k: _guarded(n, v, dev) for k, v in host.items()}
    device_scalars = {k: torch.tensor(v, dtype=torch.float64, device=dev) for k, v in scalars.items()}  # ONE element each
    want_rows = {k: v.copy() for k, v in host.items()}
    ops, want_ops, outs = [], [], []
    for op, src, source, out in PROGRAMS[name]:
        column = device_scalars[source] if source in scalars else (device[source][1] if source else None)
        want_column = scalars[source] if source in scalars else (want_rows[source] if source else None)
        if out == "new":
            whole, row = _guarded(n, None, dev)
            want = np.full(n, SENTINEL)
        elif out == "same":
            (whole, row), want = device[source], want_rows[source]
        else:
            whole = row = want = None
        ops.append((native.ROW_OPS[op], src, column, row))
        want_ops.append((R.CODES[op], src, want_column, want))
        outs.append((whole, row, want))
    native.obs_column_ops(ops, n)
    torch.cuda.synchronize()
    R.launch(want_ops, n)
    for t, (whole, row, want) in enumerate(outs):
        if row is not None:
            got = row.cpu().numpy()
            assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist(), (name, n, t, PROGRAMS[name][t])
            assert _guards_hold(whole, n), (name, n, t)
    for k, (whole, row) in device.items():  # the inputs: as they were unless written in place, and their guards hold
        assert _guards_hold(whole, n) and row.cpu().numpy().view(np.uint64).tolist() == want_rows[k].view(np.uint64).tolist(), (name, n, k)
    for k, t in device_scalars.items():
        assert t.cpu().numpy().tolist() == scalars[k].tolist()


def test_every_code_is_in_a_program_above():
    assert {op for program in PROGRAMS.values() for op, *_ in program} == set(native.ROW_OPS)
    assert all(len(program) <= native.MAX_COLUMN_OPS for program in PROGRAMS.values())


def test_argument_errors_reach_python(dev):
    x = torch.zeros(8, dtype=torch.float64, device=dev)
    for ops, message in [([(33, -1, x, x.clone())], "unknown code"), ([(native.ROW_OPS["cmp_gt"], -1, x, x.clone())], "binary"),
                         ([(native.ROW_OPS["copy"], -1, x, None), (native.COLUMN_OPS["log"], -1, x, x.clone())], "mixes the two families"),
                         ([(native.ROW_OPS["copy"], -1, x, None), (native.ROW_OPS["scalar"], 0, None, x.clone())], "SCALAR")]:
        with pytest.raises(Exception, match=message):
            native.obs_column_ops(ops, 8)


# ---- the filters against the reference's frames ----------------------------------------------------------------------------------------------
def _frame_only(case: dict) -> bool:
    return case["filter"] in R.FRAME_ONLY and any(v.dtype.kind == "O" for v in case["changed"].values())


@pytest.mark.parametrize("kind", ["frame", "host", "device"])
def test_filters_give_the_reference_frames(dev, kind):
    pytest.importorskip("pandas")
    for case in GOLDEN["cases"]:
        table = R.input_table(GOLDEN, case, kind, dev)
        f = create_filter_by_name(case["filter"], **case["config"])
        if kind != "frame" and _frame_only(case):
            with pytest.raises(ValueError, match="not numeric and has missing entries"):
                f.forward(table)
            continue
        kept = {c: (v.clone() if isinstance(v, torch.Tensor) else np.array(v, copy=True)) for c, v in dict(table).items()}
        got = f.forward(table)
        assert got is not table, case["id"]
        R.check_case(got, GOLDEN, case, kind)
        for c, v in kept.items():  # the caller's table is as it was
            now, was = table[c], v
            if isinstance(v, torch.Tensor):
                now, was = now.cpu().numpy(), v.cpu().numpy()
            assert R.same_column(np.asarray(now), was), (case["id"], c)
        if kind == "device":  # device tensors in, device tensors out, on the same device; strings alone stay on the host
            for c, v in got.items():
                assert (isinstance(v, torch.Tensor) and v.device == dev) == (c != "s"), (case["id"], c, type(v))
        elif kind == "host":
            assert all(isinstance(v, np.ndarray) for v in got.values()), case["id"]


def test_a_resident_chain_never_yields_a_host_column(dev):
    rng = np.random.default_rng(77)
    n = 3000
    table = {"date": torch.from_numpy(np.datetime64("2025-01-01", "ns").view(np.int64) + rng.integers(0, 7200, n) * 10**9).to(dev),
             "latitude": torch.from_numpy(rng.uniform(-80, 80, n)).to(dev), "longitude": torch.from_numpy(rng.uniform(-170, 170, n)).to(dev),
             "obsvalue_t": torch.from_numpy(np.where(rng.random(n) < 0.1, np.nan, 250.0 + 40.0 * rng.random(n))).to(dev),
             "reportype": torch.from_numpy(rng.integers(1, 4, n)).to(dev)}
    table = {c: torch.cat([v, v[:100]]) for c, v in table.items()}  # a hundred duplicate rows
    stages = [create_filter_by_name("drop_duplicates"), create_filter_by_name("mask_outside_range", obsvalue_t=[255.0, 285.0]),
              create_filter_by_name("drop_nans_tabular", columns=["obsvalue_t"]),
              create_filter_by_name("superob", grid="5/5", timeslot_length=3600, columns_to_take_nearest=["date"], columns_to_groupby=["reportype"])]
    seen, out = [], table
    for f in stages:
        out = f(out)
        seen.append(out)
    piped = (stages[0] | stages[1] | stages[2] | stages[3])(table)
    assert list(piped) == list(out) and all(torch.equal(piped[c], out[c]) or c != "date" for c in out)
    assert len(seen) == 4 and all(isinstance(v, torch.Tensor) and v.device == dev for stage in seen for v in stage.values())
    host = {c: v.cpu().numpy() for c, v in table.items()}
    first = np.unique(np.stack([host[c].view(np.int64) for c in host]), axis=1, return_index=True)[1]
    t = host["obsvalue_t"][np.sort(first)]
    want = int(((t >= 255.0) & (t <= 285.0)).sum())
    assert seen[0]["date"].numel() == n and seen[2]["obsvalue_t"].numel() == want and 0 < out["obsvalue_t"].numel() <= want
    assert not bool(torch.isnan(seen[2]["obsvalue_t"]).any())


def test_dispatchers_on_a_frame_and_on_a_mapping(dev):
    pd = pytest.importorskip("pandas")
    columns = {"a": np.array([0.5, np.nan, 3.0, -1.0]), "k": np.array([0, 1, 2, 3])}
    for table in (pd.DataFrame(columns, index=[7, 5, 3, 1]), columns, {c: torch.from_numpy(v).to(dev) for c, v in columns.items()}):
        def host(v):
            return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

        out = create_filter_by_name("mask", k={"value": 2, "operator": ">="}).forward(table)
        assert R.same_bits(host(out["k"]), np.array([0, 1, np.nan, np.nan])) and R.same_bits(host(out["a"]), columns["a"])
        out = create_filter_by_name("clip", a=[0.0, 1.0], k=(1, 2)).forward(table)
        assert R.same_bits(host(out["a"]), np.array([0.5, np.nan, 1.0, 0.0])) and R.same_bits(host(out["k"]), np.array([1, 1, 2, 2]))
        out = create_filter_by_name("impute_nans", value=9.0, columns=["a"]).forward(table)
        assert R.same_bits(host(out["a"]), np.array([0.5, 9.0, 3.0, -1.0])) and R.same_bits(host(out["k"]), columns["k"])
        out = create_filter_by_name("remove_nans", how="any").forward(table)
        assert R.same_bits(host(out["a"]), np.array([0.5, 3.0, -1.0])) and R.same_bits(host(out["k"]), np.array([0, 2, 3]))
        assert not hasattr(out, "index") or list(out.index) == [7, 3, 1]
        assert isinstance(out["a"], torch.Tensor) == isinstance(table["a"], torch.Tensor)
