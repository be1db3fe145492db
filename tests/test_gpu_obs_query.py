"""The row-expression kernels (csrc/atx_obs_row_expr.hip) and ``filter_query`` / ``mask_values_custom`` on the device.

- ``native.obs_row_expr`` against the plain numpy interpreter (tests/row_expr_restatement.py), bit for bit: every instruction code,
  operands from columns, constants and the stack, the stack at its full depth of 8, an ``IN_SET`` of 1 and of 64 members, value rows in
  place over an input; n = 0, 1, 63, 64, 65, 255, 256, 257 (one lane, the edges of a wave and of a chunk) and ``kRowGrid * kBlock + 65``,
  where a lane takes a second row; guard elements before and after every input, value row, word row, count row and position row.
- Keep bits, chunk counts and ``native.obs_keep_positions`` for four keep patterns at the same sizes.
- ``ROUND_F32`` against numpy's float32 arithmetic on subnormals, halfway cases and overflow.
- Every ``ATX_EINVAL`` condition as a Python exception, nothing written.
- Both filters against the frames the reference itself returned (tests/golden/obs_query.json) on a DataFrame, a dict of arrays and a dict
  of device tensors; a resident chain through both.
At ``kRowGrid * kBlock + 65`` rows (2 GB per float64 row) the rows are made on the device and the 2 GB results are compared there, against
torch's own IEEE arithmetic and ``torch.nonzero``; the words and counts, and windows of the rows at both ends and at the grid's seam, go
through the numpy restatement like every other size.  Everything is exact: there is no tolerance in this file.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import row_expr_restatement as X
import row_program_restatement as R
from anemoi_transform_amd import native
from anemoi_transform_amd.filters import create_filter_by_name

pytestmark = pytest.mark.gpu
GOLDEN = X.load_golden()
GRID_ROWS = (1 << 20) * 256  # kRowGrid * kBlock
BIG = GRID_ROWS + 65
SIZES = tuple(dict.fromkeys((0, 1, 63, 64, 65, 257, native.EXPR_CHUNK_ROWS - 1, native.EXPR_CHUNK_ROWS, native.EXPR_CHUNK_ROWS + 1)))  # 257 once
SENTINEL = -12345.678
INT_SENTINEL = -0x0123456789ABCDEF
PAYLOAD_NAN = np.array([0x7FF4000000ABCDEF, 0xFFF8000000000001], dtype=np.uint64).view(np.float64)
POOL = np.concatenate([PAYLOAD_NAN, R.value_pool()])
CONSTS = tuple([2.5, 0.1] + [float(v) for v in R.value_pool() if v == v][:40] + [float(k) for k in range(22)])  # 64 of them
assert len(CONSTS) == native.EXPR_MAX_CONSTS

# name -> (code, inputs read, value results, keep, {result: input it is written over})
PROGRAMS = {
    "arithmetic": ([("push_col", 0), ("push_col", 1), ("add",), ("push_const", 0), ("mul",), ("push_col", 2), ("sub",), ("push_col", 0), ("div",), ("neg",),
                    ("abs",), ("round_f32",)], 3, 1, False, {}),
    "compares": ([("push_col", 0), ("push_col", 1), ("cmp_gt",), ("push_col", 0), ("push_const", 0), ("cmp_lt",), ("or",), ("push_col", 1), ("push_col", 2),
                  ("cmp_eq",), ("push_col", 0), ("push_col", 2), ("cmp_ne",), ("and",), ("or",), ("push_col", 0), ("push_const", 1), ("cmp_ge",),
                  ("push_col", 2), ("push_col", 1), ("cmp_le",), ("and",), ("not",), ("or",)], 3, 0, True, {}),
    "sets": ([("push_col", 0), ("in_set", 0, 1), ("push_col", 1), ("in_set", 0, 64), ("or",), ("push_col", 2), ("in_set", 5, 3), ("not",), ("and",)],
             3, 0, True, {}),
    # eight deep, operands taken from the stack; x and v are written in place, v masked
    "full_stack": ([("push_col", 0), ("push_col", 1), ("push_col", 2), ("push_const", 0), ("push_const", 1), ("dup", 4), ("dup", 3), ("dup", 0), ("add",),
                    ("swap",), ("sub",), ("mul",), ("cmp_lt",), ("nan_where",), ("dup", 1), ("push_const", 0), ("cmp_gt",)], 3, 3, True, {0: 0, 2: 2}),
    "truth_of_any_value": ([("push_col", 0), ("push_col", 1), ("and",), ("push_col", 2), ("not",), ("or",), ("push_col", 0), ("dup", 1), ("nan_where",),
                            ("swap",)], 3, 1, True, {}),
    "one_column": ([("push_col", 0)], 1, 1, False, {}),
    "one_constant": ([("push_const", 7)], 0, 1, False, {}),
    "a_column_as_its_own_condition": ([("push_col", 0)], 1, 0, True, {}),
    "four_results": ([("push_col", 0), ("push_col", 1), ("push_col", 2), ("dup", 2), ("dup", 2), ("div",)], 3, 4, False, {3: 1}),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    d = torch.device("cuda", 0)
    torch.cuda.set_device(d)
    native.load()
    return d


def _code(program) -> list[tuple[int, int, int]]:
    return [(native.EXPR_OPS[i[0]], i[1] if len(i) > 1 else 0, i[2] if len(i) > 2 else 0) for i in program]


def _rows(n: int, k: int = 3) -> list[np.ndarray]:
    """Rows of n values: the specials (payload NaNs, both zeros, infinities, values on and beside the constants) first, random beyond."""
    rng = np.random.default_rng(5200 + n)
    out = []
    for _ in range(k):
        a = np.where(rng.random(n) < 0.4, rng.choice(POOL, n), np.round(rng.standard_normal(n) * 3.0, 1))
        a[:min(n, len(POOL))] = rng.permutation(POOL)[:n]
        out.append(a)
    return out


def _guarded(n: int, values=None, dev=None, dtype=torch.float64):
    whole = torch.full((n + 128,), SENTINEL if dtype == torch.float64 else INT_SENTINEL, dtype=dtype, device=dev)
    row = whole[32:32 + n]
    if values is not None:
        row.copy_(torch.from_numpy(np.ascontiguousarray(values).view(np.int64).copy()).view(dtype))  # the bits, whatever a copy does with a signalling NaN
    return whole, row


def _guards_hold(whole: torch.Tensor, n: int) -> bool:
    sentinel = SENTINEL if whole.dtype == torch.float64 else INT_SENTINEL
    return bool((whole[:32] == sentinel).all()) and bool((whole[32 + n:] == sentinel).all())


def _bits(t: torch.Tensor) -> list:
    return t.cpu().numpy().view(np.uint64).tolist()


# (program, result) whose value comes out of + - * / or ROUND_F32: where it is a NaN, IEEE leaves sign and payload to the implementation
# (numpy's host gives inf - inf a negative NaN), so a NaN there is compared as a NaN; every other result is compared on its bits.
COMPUTED = {("arithmetic", 0), ("four_results", 3)}


def _same(got: torch.Tensor, want: np.ndarray, computed: bool = False) -> bool:
    g = got.cpu().numpy()
    if computed:
        value = ~np.isnan(want)
        return np.array_equal(np.isnan(g), ~value) and g[value].view(np.uint64).tolist() == want[value].view(np.uint64).tolist()
    return g.view(np.uint64).tolist() == want.view(np.uint64).tolist()


def _launch(dev, code, host_inputs, n, n_results, keep, alias=None):
    """One launch over guarded rows: ``(inputs, outs, words, counts)`` as ``(whole, row)`` pairs."""
    inputs = [_guarded(n, v, dev) for v in host_inputs]
    outs = [inputs[alias[r]] if r in (alias or {}) else _guarded(n, None, dev) for r in range(n_results)]
    words = _guarded((n + 63) // 64, None, dev, torch.int64) if keep else None
    counts = _guarded((n + native.EXPR_CHUNK_ROWS - 1) // native.EXPR_CHUNK_ROWS, None, dev, torch.int64) if keep else None
    native.obs_row_expr(_code(code), [row for _, row in inputs], CONSTS, [row for _, row in outs], n,
                        keep_words=words[1] if keep else None, chunk_counts=counts[1] if keep else None)
    torch.cuda.synchronize()
    return inputs, outs, words, counts


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_kernel_against_the_interpreter(dev, name, n):
    code, k, n_results, keep, alias = PROGRAMS[name]
    host = _rows(n, k)
    inputs, outs, words, counts = _launch(dev, code, host, n, n_results, keep, alias)
    left = X.run(_code(code), host, CONSTS, n)
    assert len(left) == n_results + keep
    for r, (whole, row) in enumerate(outs):
        assert _same(row, left[r], (name, r) in COMPUTED), (name, n, r)
        assert _guards_hold(whole, n), (name, n, r)
    for j, (whole, row) in enumerate(inputs):  # as they were unless written in place
        if j not in alias.values():
            assert _bits(row) == host[j].view(np.uint64).tolist(), (name, n, j)
        assert _guards_hold(whole, n), (name, n, j)
    if keep:
        kept = left[-1] != 0
        assert _bits(words[1]) == X.pack_words(kept).tolist() and _guards_hold(words[0], (n + 63) // 64), (name, n)
        assert counts[1].cpu().numpy().tolist() == X.chunk_counts(kept).tolist() and _guards_hold(counts[0], counts[1].numel()), (name, n)


def test_every_code_is_in_a_program_above():
    assert {i[0] for program, *_ in PROGRAMS.values() for i in program} == set(native.EXPR_OPS)
    assert all(len(program) <= native.EXPR_MAX_INSTR for program, *_ in PROGRAMS.values())
    assert len(X.run(_code(PROGRAMS["full_stack"][0][:8]), _rows(4), CONSTS, 4)) == 8 == native.EXPR_MAX_STACK == X.MAX_STACK  # eight pushes
    assert ("in_set", 0, 1) in PROGRAMS["sets"][0] and ("in_set", 0, 64) in PROGRAMS["sets"][0]
    assert X.CODES == native.EXPR_OPS and X.CHUNK_ROWS == native.EXPR_CHUNK_ROWS


def test_the_grid_stride_loop_runs_a_second_time(dev):
    """``kRowGrid * kBlock + 65`` rows: the first 65 lanes of the launch take a second row.  x = 0, 1, 2, ... made on the device; the value
    row is x * 2.5, the keep condition x * 2.5 > 5.  The 2 GB value row is compared on the device with torch's product (IEEE's, as
    numpy's), the words and counts with the packing of torch's compare, and windows at both ends and across the seam with the
    restatement."""
    n = BIG
    code = [("push_col", 0), ("push_const", 0), ("mul",), ("dup", 0), ("push_const", 47), ("cmp_gt",)]
    assert CONSTS[0] == 2.5 and CONSTS[47] == 5.0
    whole, x = _guarded(n, None, dev)
    torch.arange(n, dtype=torch.float64, out=x)
    out_whole, out = _guarded(n, None, dev)
    words_whole, words = _guarded((n + 63) // 64, None, dev, torch.int64)
    counts_whole, counts = _guarded((n + 255) // 256, None, dev, torch.int64)
    native.obs_row_expr(_code(code), [x], CONSTS, [out], n, keep_words=words, chunk_counts=counts)
    torch.cuda.synchronize()
    assert all(_guards_hold(w, m) for w, m in ((whole, n), (out_whole, n), (words_whole, words.numel()), (counts_whole, counts.numel())))
    assert torch.equal(x, torch.arange(n, dtype=torch.float64, device=dev))
    assert torch.equal(out, x * 2.5)
    kept = (out > 5.0).cpu().numpy()
    assert not kept[:3].any() and kept[3:].all()
    got_words = words.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_words, X.pack_words(kept)) and np.array_equal(counts.cpu().numpy(), X.chunk_counts(kept))
    for lo, hi in ((0, 65536), (GRID_ROWS - 65536, n)):  # both ends, and the seam where the second trip starts
        left = X.run(_code(code), [np.arange(lo, hi, dtype=np.float64)], CONSTS, hi - lo)
        assert out[lo:hi].cpu().numpy().view(np.uint64).tolist() == left[0].view(np.uint64).tolist()
        assert np.array_equal(got_words[lo // 64:(hi + 63) // 64], X.pack_words(left[1] != 0))


# ---- keep bits and positions -------------------------------------------------------------------------------------------------------------------
PATTERNS = ("all", "none", "every_64th", "half")


def _pattern(name: str, n: int, dev) -> torch.Tensor:
    if name == "all":
        return torch.ones(n, dtype=torch.bool, device=dev)
    if name == "none":
        return torch.zeros(n, dtype=torch.bool, device=dev)
    if name == "every_64th":
        return torch.arange(n, device=dev) % 64 == 63
    return torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(64 + n % 1000)) < 0.5


@pytest.mark.parametrize("n", SIZES + (BIG,))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_keep_bits_counts_and_positions(dev, pattern, n):
    mask = _pattern(pattern, n, dev)
    whole, m = _guarded(n, None, dev)
    m.copy_(mask * 2.5)  # any value that is not 0 keeps the row
    n_words, n_chunks = (n + 63) // 64, (n + native.EXPR_CHUNK_ROWS - 1) // native.EXPR_CHUNK_ROWS
    words_whole, words = _guarded(n_words, None, dev, torch.int64)
    counts_whole, counts = _guarded(n_chunks, None, dev, torch.int64)
    native.obs_row_expr(_code([("push_col", 0)]), [m], (), [], n, keep_words=words, chunk_counts=counts)
    host = mask.cpu().numpy()
    want = np.flatnonzero(host)
    assert np.array_equal(words.cpu().numpy().view(np.uint64), X.pack_words(host))
    if n % 64:
        assert int(words[-1].cpu().numpy().view(np.uint64)) >> (n % 64) == 0  # the padding bits
    assert np.array_equal(counts.cpu().numpy(), X.chunk_counts(host)) and int(counts.sum()) == len(want)
    ends = torch.cumsum(counts, 0)
    total = int(ends[-1]) if n else 0
    assert total == len(want)
    where_whole, where = _guarded(total, None, dev, torch.int64)
    native.obs_keep_positions(words, ends - counts if n else counts, n, where)
    torch.cuda.synchronize()
    if n <= GRID_ROWS:
        assert np.array_equal(where.cpu().numpy(), want)
    else:  # 2 GB of positions: compared on the device, and the ends on the host
        assert torch.equal(where, torch.nonzero(mask).reshape(-1))
        assert np.array_equal(where[:70000].cpu().numpy(), want[:70000]) and np.array_equal(where[-70000:].cpu().numpy(), want[len(want) - 70000:])
    assert all(_guards_hold(w, k) for w, k in ((whole, n), (words_whole, n_words), (counts_whole, n_chunks), (where_whole, total)))
    assert torch.equal(m, mask.to(torch.float64) * 2.5)


# ---- ROUND_F32 ---------------------------------------------------------------------------------------------------------------------------------
def _f32_pool() -> np.ndarray:
    tiny, fmax = 2.0 ** -149, float(np.finfo(np.float32).max)
    pool = [0.0, -0.0, np.nan, np.inf, -np.inf, tiny, tiny / 2, 3 * tiny / 2, np.nextafter(tiny / 2, 1.0), np.nextafter(tiny / 2, 0.0), 5 * tiny / 2,
            2.0 ** -126, 2.0 ** -126 - tiny / 2, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, np.nextafter(1.0 + 2.0 ** -24, 2.0), 1.0 - 2.0 ** -25,
            fmax, fmax + 2.0 ** 103, np.nextafter(fmax + 2.0 ** 103, 0.0), 1e39, -1e39, 0.1, 1.0 / 3.0, 16777217.0, 5e-324, 1e-40, -1e-45]
    return np.array(pool, dtype=np.float64)


def test_round_f32_is_numpys_float32(dev):
    pool = _f32_pool()
    inputs, outs, _, _ = _launch(dev, [("push_col", 0), ("round_f32",)], [pool], len(pool), 1, False)
    with np.errstate(over="ignore", invalid="ignore"):
        want = pool.astype(np.float32)
    assert _same(outs[0][1], want.astype(np.float64), True)
    fmax = float(np.finfo(np.float32).max)
    at = {v: k for k, v in enumerate(pool.tolist()) if v == v}
    assert np.isinf(want[at[fmax + 2.0 ** 103]]) and want[at[float(np.nextafter(fmax + 2.0 ** 103, 0.0))]] == np.float32(fmax)  # the tie goes to even: inf
    assert want[at[2.0 ** -150]] == 0 and want[at[3 * 2.0 ** -150]] == np.float32(2.0 ** -148) and want[at[1.0 + 2.0 ** -24]] == 1  # ties to even
    # + - * / of float32 operands, each rounded once more: numpy's float32 results, subnormal ones included
    rng = np.random.default_rng(32)
    f32 = np.concatenate([want[np.isfinite(want)], rng.standard_normal(200).astype(np.float32), (rng.standard_normal(200) * 1e-38).astype(np.float32),
                          (rng.standard_normal(100) * 1e-22).astype(np.float32), (rng.standard_normal(100) * 1e19).astype(np.float32)])
    x, y = np.meshgrid(f32, f32[::7])
    x, y = x.reshape(-1), y.reshape(-1)
    code = [i for op in ("add", "sub", "mul", "div") for i in (("push_col", 0), ("push_col", 1), (op,), ("round_f32",))]
    _, outs, _, _ = _launch(dev, code, [x.astype(np.float64), y.astype(np.float64)], len(x), 4, False)
    with np.errstate(all="ignore"):
        wants = [x + y, x - y, x * y, x / y]
    assert any(((w != 0) & (np.abs(w) < 2.0 ** -126)).any() for w in wants)  # subnormal results are among them
    for (_, row), w in zip(outs, wants):
        got = row.cpu().numpy()
        assert w.dtype == np.float32
        value = ~np.isnan(w)  # a NaN result carries whatever payload the operation gives it: NaN where numpy has NaN
        assert np.array_equal(np.isnan(got), ~value) and got[value].view(np.uint64).tolist() == w[value].astype(np.float64).view(np.uint64).tolist()


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_reach_python(dev):
    from ctypes import c_double, c_int32, c_void_p

    n = 8
    whole, x = _guarded(n, np.arange(8.0), dev)
    out_whole, out = _guarded(n, None, dev)
    many = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(17)]
    words = torch.zeros(1, dtype=torch.int64, device=dev)
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    push, add, in_set = ("push_col", 0), ("add",), native.EXPR_OPS["in_set"]
    bad = [
        ([push] * 33, [x], (), [out], "instructions"), ([push] * 34, [x], (), [out] * 4, "instructions"),
        ([("push_col", k) for k in range(17)], many, (), [out], "input columns"), ([push, (in_set, 0, 65)], [x], [0.0] * 65, [out], "constants"),
        ([push] * 5, [x], (), [out] * 5, "value results"), ([push], [x], (), [], "neither"), ([(22, 0, 0)], [x], (), [out], "unknown code"),
        ([push, (-1, 0, 0)], [x], (), [out], "unknown code"), ([push, add], [x], (), [out], "underflow"), ([("swap",)], [x], (), [out], "underflow"),
        ([("dup", 1)], [x], (), [out], "underflow"), ([push] * 9 + [add] * 8, [x], (), [out], "overflow"), ([push, push], [x], (), [out], "leaves 2 values"),
        ([push], [x], (), [out, out], "leaves 1 values"), ([("push_col", 1)], [x], (), [out], "column 1 of 1"), ([("push_col", -1)], [x], (), [out], "column -1"),
        ([("push_const", 2)], [x], [1.0, 2.0], [out], "constant 2 of 2"), ([push, (in_set, 1, 2)], [x], [1.0, 2.0], [out], "IN_SET"),
        ([push, (in_set, 0, 0)], [x], [1.0, 2.0], [out], "IN_SET"), ([push, (in_set, -1, 1)], [x], [1.0, 2.0], [out], "IN_SET"),
        ([push], [None], (), [out], "null input column"), ([push], [x], (), [None], "output row 0 is null"),
    ]
    for code, inputs, consts, outs, message in bad:
        code = [(native.EXPR_OPS[i[0]] if isinstance(i[0], str) else i[0], *(list(i[1:]) + [0, 0])[:2]) for i in code]
        with pytest.raises(ValueError, match=message):
            native.obs_row_expr(code, inputs, consts, outs, n)
    with pytest.raises(ValueError, match="leaves 1 values"):  # a keep condition needs a slot of its own
        native.obs_row_expr([(0, 0, 0)], [x], (), [out], n, keep_words=words, chunk_counts=counts)
    with pytest.raises(ValueError, match="go together"):
        native.obs_row_expr([(0, 0, 0)], [x], (), [], n, keep_words=words)
    # the entry points themselves, on the device rows: what the wrappers cannot say
    px, po, pw, pc = x.data_ptr(), out.data_ptr(), words.data_ptr(), counts.data_ptr()
    zero, none = (c_int32 * 1)(0), (c_void_p * 1)(None)

    def flat(rows=n, keep=0, keep_words=None, chunk_counts=None, **instead):  # the program [push_col 0] over x: one result, or a keep condition alone
        args = {"code": zero, "arg0": zero, "arg1": zero, "in": (c_void_p * 1)(px), "consts": (c_double * 1)(0.0), "out": none if keep else (c_void_p * 1)(po)}
        assert set(instead) <= set(args)
        args.update(instead)
        return ("atx_obs_row_expr", 1, args["code"], args["arg0"], args["arg1"], 1, args["in"], 0, args["consts"], 0 if keep else 1, args["out"], keep,
                keep_words, chunk_counts, rows, None)

    for call, message in [(flat(code=None), "null program array"), (flat(arg0=None), "null program array"), (flat(arg1=None), "null program array"),
                          (flat(rows=-1), "-1 rows"), (flat(**{"in": None}), "null table"), (flat(out=None), "null table"),
                          (flat(keep=1, keep_words=None, chunk_counts=pc), "null keep_words or chunk_counts"),
                          (flat(keep=1, keep_words=pw, chunk_counts=None), "null keep_words or chunk_counts"),
                          (("atx_obs_keep_positions", pw, pc, -1, po, 1, None), "-1 rows"), (("atx_obs_keep_positions", pw, pc, n, po, -1, None), "-1 positions"),
                          (("atx_obs_keep_positions", None, pc, n, po, 1, None), "null pointer"), (("atx_obs_keep_positions", pw, None, n, po, 1, None), "null pointer"),
                          (("atx_obs_keep_positions", pw, pc, n, None, 1, None), "null pointer")]:
        with pytest.raises(ValueError, match=message):
            native._call(*call)
    native.obs_row_expr([(0, 0, 0)], [x[:0]], (), [out[:0]], 0)  # n == 0: validated, nothing launched
    native._call(*flat(rows=0, keep=1, **{"in": none}))
    native._call("atx_obs_keep_positions", None, None, 0, None, 0, None)
    torch.cuda.synchronize()
    assert bool((out_whole == SENTINEL).all()) and _guards_hold(whole, n) and x.cpu().numpy().tolist() == list(range(8))  # nothing was launched
    assert int(words[0]) == 0 and int(counts[0]) == 0


# ---- the filters against the reference's frames -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["frame", "host", "device"])
def test_filters_give_the_reference_frames(dev, kind):
    pytest.importorskip("pandas")
    for case in GOLDEN["cases"]:
        table = R.input_table(GOLDEN, case, kind, dev)
        f = create_filter_by_name(case["filter"], **case["config"])
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
                stays = isinstance(table[c], np.ndarray)  # the string column of the table, if it has one
                assert stays == (np.asarray(GOLDEN["tables"][case["table"]]["columns"][c]).dtype.kind == "O")
                assert (isinstance(v, torch.Tensor) and v.device == dev) != stays and (isinstance(v, np.ndarray) == stays), (case["id"], c, type(v))
        elif kind == "host":
            assert all(isinstance(v, np.ndarray) for v in got.values()), case["id"]


def test_a_resident_chain_never_yields_a_host_column(dev):
    rng = np.random.default_rng(78)
    n = 3000
    table = {"date": torch.from_numpy(np.datetime64("2025-01-01", "ns").view(np.int64) + rng.integers(0, 7200, n) * 10**9).to(dev),
             "latitude": torch.from_numpy(rng.uniform(-80, 80, n)).to(dev), "longitude": torch.from_numpy(rng.uniform(-170, 170, n)).to(dev),
             "obsvalue_t": torch.from_numpy(250.0 + 40.0 * rng.random(n)).to(dev), "pressure": torch.from_numpy(rng.choice([85000.0, 50000.0, 30000.0], n)).to(dev),
             "varno": torch.from_numpy(rng.choice([1, 2, 7, 59], n)).to(dev), "reportype": torch.from_numpy(rng.integers(1, 4, n)).to(dev)}
    table = {c: torch.cat([v, v[:100]]) for c, v in table.items()}  # a hundred duplicate rows
    stages = [create_filter_by_name("drop_duplicates"), create_filter_by_name("filter_query", query="varno in [1, 2, 7] and pressure > 40000"),
              create_filter_by_name("mask_values_custom", obsvalue_t="abs(obsvalue_t - 270) > 15 & pressure < 60000"),
              create_filter_by_name("superob", grid="5/5", timeslot_length=3600, columns_to_take_nearest=["date"], columns_to_groupby=["reportype"])]
    seen, out = [], table
    for f in stages:
        out = f(out)
        seen.append(out)
    piped = (stages[0] | stages[1] | stages[2] | stages[3])(table)
    assert list(piped) == list(out) and all(torch.equal(piped[c].view(torch.int64), out[c].view(torch.int64)) for c in out)
    assert len(seen) == 4 and all(isinstance(v, torch.Tensor) and v.device == dev for stage in seen for v in stage.values())
    host = {c: v.cpu().numpy()[:n] for c, v in table.items()}
    keep = np.isin(host["varno"], [1, 2, 7]) & (host["pressure"] > 40000)
    assert seen[0]["date"].numel() == n and seen[1]["varno"].numel() == int(keep.sum())
    t = host["obsvalue_t"][keep]
    want = np.where((np.abs(t - 270) > 15) & (host["pressure"][keep] < 60000), np.nan, t)
    assert R.same_bits(seen[2]["obsvalue_t"].cpu().numpy(), want) and np.isnan(want).any() and 0 < out["obsvalue_t"].numel() <= len(want)
