"""The output store of the column gather kernels (``store_out``, csrc/atx_regrid_decl.hpp), whatever cache policy it carries: every
element it must write holds the bits of the chain computed in numpy in the statement's order — ``(((0 + w0*v0) + w1*v1) + w2*v2) + w3*v3``,
a rounded product then a rounded sum, no FMA — every byte it must not write keeps its sentinel, and what it wrote is what the next kernel
on the stream and the host see.

The pair is synthetic: 1 000 source points, 777 targets, random indices.  777 x C is not a multiple of the 256-lane workgroup, so the
last workgroup of a launch is partial; an odd level count leaves a pad element in the last 16-byte vector, which the vector route writes
(the chain of the source's pad elements) and the scalar route does not.  The output is a view into a larger buffer full of a sentinel:
``tight`` puts the base on a 128-byte line with the pitch the levels need; ``loose`` puts it 16 bytes past a line, so every wave's
store straddles lines, with a pitch one vector wider, so every row leaves a hole; ``scalar`` has a pitch that is no multiple of 16 bytes,
which takes the one-element instantiations and their 8- and 4-byte stores.  The field-major fixed-k kernel, whose store is written
through, gets the same frame with a row per level."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from anemoi_transform_amd import native

pytestmark = pytest.mark.gpu

N_SRC, N_TGT = 1000, 777
SENTINEL = 0xA5
GUARD = 64  # elements of sentinel after the last row
DTYPES = {"f32": (torch.float32, np.float32, np.uint32), "f64": (torch.float64, np.float64, np.uint64)}


def vec_of(t: str) -> int:
    return 16 // np.dtype(DTYPES[t][1]).itemsize


def covered(t: str, n_lev: int) -> int:
    vec = vec_of(t)
    return (n_lev + vec - 1) // vec * vec


@functools.lru_cache(maxsize=None)
def tables(seed: int = 0):
    """Indices and float64 weights of the pair, and ragged row lengths of 1-4 for the padded and CSR forms; made once, read only."""
    rng = np.random.default_rng(20261020 + seed)
    idx = rng.integers(0, N_SRC, size=(N_TGT, 4)).astype(np.int32)
    w = rng.uniform(0.05, 1.0, size=(N_TGT, 4))
    w /= w.sum(axis=1, keepdims=True)
    lengths = rng.integers(1, 5, size=N_TGT)
    for a in (idx, w, lengths):
        a.setflags(write=False)
    return idx, w, lengths


@functools.lru_cache(maxsize=None)
def source(t: str, n_lev: int, seed: int = 0) -> np.ndarray:
    """(N_SRC, covered levels) of the stack's type, pad elements included: the vector route gathers them too."""
    rng = np.random.default_rng(7 + 13 * n_lev + seed)
    a = (250.0 + 30.0 * rng.standard_normal((N_SRC, covered(t, n_lev)))).astype(DTYPES[t][1])
    a.setflags(write=False)
    return a


def chain(src: np.ndarray, idx: np.ndarray, w: np.ndarray | None) -> np.ndarray:
    """The statement of the kernels on the host: a pure gather is a copy; otherwise the sum starts at 0 and takes ``acc + w * v`` entry by
    entry, each product and each sum rounded to the stack's type; a negative index is an absent entry."""
    if w is None:
        return src[idx[:, 0]].copy()
    acc = np.zeros((idx.shape[0], src.shape[1]), dtype=src.dtype)
    for j in range(idx.shape[1]):
        present = idx[:, j] >= 0
        term = w[:, j, None].astype(src.dtype) * src[np.where(present, idx[:, j], 0)]
        acc = np.where(present[:, None], acc + term, acc)
    return acc


class Frame:
    """An output view inside a sentinel-filled device buffer, and the host's picture of what the buffer must hold afterwards."""

    def __init__(self, dev, t: str, n_lev: int, layout: str, n_rows: int = N_TGT):
        tdt, npdt, self.bits = DTYPES[t]
        vec, item = vec_of(t), np.dtype(npdt).itemsize
        self.n_rows, self.n_lev = n_rows, n_lev
        if layout == "tight":
            lead, self.pitch, self.width = 0, covered(t, n_lev), covered(t, n_lev)
        elif layout == "loose":
            lead, self.pitch, self.width = 16 // item, covered(t, n_lev) + vec, covered(t, n_lev)
        elif layout == "fields":  # field-major: a row per level, N_TGT elements of it written, three more in the pitch
            self.n_rows = n_rows = n_lev
            lead, self.pitch, self.width = 16 // item, N_TGT + 3, N_TGT
        else:  # scalar: the smallest pitch above the levels that is no whole number of vectors; exactly the levels are written
            assert layout == "scalar"
            lead, self.pitch, self.width = 16 // item, n_lev + 1 + (1 if (n_lev + 1) % vec == 0 else 0), n_lev
        self.lead = lead
        total = lead + n_rows * self.pitch + GUARD
        raw = torch.full((total * item,), SENTINEL, dtype=torch.uint8, device=dev)
        assert raw.data_ptr() % 128 == 0
        self.buf = raw.view(tdt)
        self.out = self.buf[lead:lead + n_rows * self.pitch]
        assert (self.out.data_ptr() % 128 == 16) == (layout != "tight")
        self.want = np.full(total * item, SENTINEL, dtype=np.uint8).view(self.bits)

    def expect(self, rows: np.ndarray, order: np.ndarray | None = None) -> "Frame":
        """``rows`` (n_rows, >= width): table row i lands in output row ``order[i]``."""
        view = self.want[self.lead:self.lead + self.n_rows * self.pitch].reshape(self.n_rows, self.pitch)
        view[np.arange(self.n_rows) if order is None else order, :self.width] = np.ascontiguousarray(rows[:, :self.width]).view(self.bits)
        return self

    def check(self, what: str) -> None:
        got = self.buf.cpu().numpy().view(self.bits)
        bad = np.flatnonzero(got != self.want)
        assert bad.size == 0, (f"{what}: {bad.size} elements differ, first at buffer element {bad[0]} (row {(bad[0] - self.lead) // self.pitch}, "
                               f"column {(bad[0] - self.lead) % self.pitch} of pitch {self.pitch}): {got[bad[0]]:#x}, expected {self.want[bad[0]]:#x}")


def device_source(dev, t: str, n_lev: int, seed: int = 0):
    """The source stack on the device; its pitch is the covered width, a whole number of vectors."""
    return torch.from_numpy(source(t, n_lev, seed).copy()).to(dev).reshape(-1), covered(t, n_lev)


def device_tables(dev, t: str, k: int, idx: np.ndarray, w: np.ndarray):
    return (torch.from_numpy(np.array(idx[:, :k])).to(dev),
            None if k == 1 else torch.from_numpy(np.array(w[:, :k], dtype=DTYPES[t][1])).to(dev))


def ell(dev, t, n_lev, k, frame, *, idx=None, w=None, seed=0, **kw):
    """One fixed-k launch into ``frame``; returns the numpy chain of the same tables over the covered width."""
    idx0, w0, _ = tables()
    idx, w = (idx0 if idx is None else idx)[:, :k], (w0 if w is None else w)[:, :k]
    src_d, sp = device_source(dev, t, n_lev, seed)
    idx_d, w_d = device_tables(dev, t, k, idx, w)
    native.regrid_ell(src_d, frame.out, idx_d, w_d, n_src=N_SRC, n_tgt=N_TGT, k=k, n_lev=n_lev, src_pitch=sp, out_pitch=frame.pitch,
                      layout=native.COLUMNS, **kw)
    return chain(source(t, n_lev, seed), idx, None if k == 1 else w.astype(DTYPES[t][1]))


@pytest.fixture
def tuning():
    try:
        yield native.set_tuning
    finally:
        native.set_tuning(0)


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("n_lev", [1, 2, 3, 137])
@pytest.mark.parametrize("layout", ["tight", "loose", "scalar"])
def test_direct_kernel_writes_the_chain_and_nothing_else(dev, layout, n_lev, k, t):
    """The edges of the launch (1, 2, 3 and 137 levels, a partial last workgroup, a pad element in the last vector), whole-line rows,
    rows that straddle lines and leave holes, and the 8- and 4-byte stores of the scalar route: the chain's bits, sentinels untouched."""
    frame = Frame(dev, t, n_lev, layout)
    want = ell(dev, t, n_lev, k, frame)
    route = native.last_gather_route()
    assert route.startswith(f"cols_ell/direct/none/{'scalar' if layout == 'scalar' else 'vec'}/k{k}/"), route
    frame.expect(want).check(route)


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("layout", ["loose", "scalar"])
def test_a_batch_of_two_stacks_stores_each_into_its_own_output(dev, layout, t):
    """grid.y = stack: two sources, two framed outputs, one launch."""
    n_lev, k = 3, 4
    idx, w, _ = tables()
    frames = [Frame(dev, t, n_lev, layout) for _ in range(2)]
    srcs = [device_source(dev, t, n_lev, seed)[0] for seed in (0, 1)]
    idx_d, w_d = device_tables(dev, t, k, idx, w)
    native.regrid_ell_batch(srcs, [f.out for f in frames], idx_d, w_d, n_src=N_SRC, n_tgt=N_TGT, k=k, n_lev=n_lev,
                            src_pitch=covered(t, n_lev), out_pitch=frames[0].pitch, layout=native.COLUMNS)
    route = native.last_gather_route()
    assert route.startswith("cols_ell/direct/"), route
    for seed, f in enumerate(frames):
        f.expect(chain(source(t, n_lev, seed), idx, w.astype(DTYPES[t][1]))).check(f"{route}, stack {seed}")


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("layout", ["loose", "scalar"])
def test_an_ordered_traversal_stores_row_t_at_tgt_rows_t(dev, layout, t):
    n_lev = 137
    order = np.random.default_rng(5).permutation(N_TGT).astype(np.int32)
    frame = Frame(dev, t, n_lev, layout)
    want = ell(dev, t, n_lev, 4, frame, tgt_rows=torch.from_numpy(order).to(dev))
    route = native.last_gather_route()
    assert route.startswith("cols_ell/direct/") and route.endswith("/ordered"), route
    frame.expect(want, order).check(route)


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("layout", ["loose", "scalar"])
def test_padded_ragged_rows_skip_their_absent_entries(dev, layout, t):
    """k = 4 with -1 entries (rows of 1-4 entries padded at the end); the weight of an absent entry is whatever the table holds."""
    n_lev = 137
    idx0, w, lengths = tables()
    idx = np.where(np.arange(4)[None, :] < lengths[:, None], idx0, -1).astype(np.int32)
    frame = Frame(dev, t, n_lev, layout)
    want = ell(dev, t, n_lev, 4, frame, idx=idx, padded=True)
    route = native.last_gather_route()
    assert route.startswith("cols_ell/direct/") and "/padded/" in route, route
    frame.expect(want).check(route)


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("layout", ["loose", "scalar"])
def test_a_by_value_epilogue_stores_the_operators_result(dev, layout, t):
    """AFFINE on every level travels by value (the uniform route): ``(x * p0) + p1``, two roundings, after the chain."""
    n_lev, npdt = 137, DTYPES[t][1]
    prog = native.level_program([[(native.OP_AFFINE, 0, 1.5, -273.25)] * n_lev], dev)
    frame = Frame(dev, t, n_lev, layout)
    want = ell(dev, t, n_lev, 4, frame, prog=prog, n_stage=1)
    route = native.last_gather_route()
    assert route.startswith("cols_ell/direct/uniform/"), route
    frame.expect(want * npdt(1.5) + npdt(-273.25)).check(route)


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("layout", ["loose", "scalar"])
def test_tiled_kernel_stores_inside_its_loop(dev, tuning, layout, t):
    """atx_set_tuning(tile=16): 16 targets x C vectors per workgroup, several stores per lane, the data registers rewritten in between."""
    n_lev = 137
    tuning(16)
    frame = Frame(dev, t, n_lev, layout)
    want = ell(dev, t, n_lev, 4, frame)
    route = native.last_gather_route()
    assert route.startswith("cols_ell/tiled/none/"), route
    frame.expect(want).check(route)


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("layout", ["loose", "scalar"])
def test_csr_kernel_stores_inside_its_loop(dev, layout, t):
    """A ragged CSR with rows of 3-4 entries, summed in storage order from 0."""
    n_lev, npdt = 137, DTYPES[t][1]
    idx, w, lengths = tables()
    keep = np.arange(4)[None, :] < np.maximum(lengths, 3)[:, None]
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    src_d, sp = device_source(dev, t, n_lev)
    frame = Frame(dev, t, n_lev, layout)
    native.regrid_csr(src_d, frame.out, torch.from_numpy(indptr).to(dev), torch.from_numpy(idx[keep]).to(dev),
                      torch.from_numpy(w[keep].astype(npdt)).to(dev), n_src=N_SRC, n_tgt=N_TGT, nnz=int(keep.sum()), n_lev=n_lev, src_pitch=sp,
                      out_pitch=frame.pitch, layout=native.COLUMNS)
    route = native.last_gather_route()
    assert route.startswith("cols_csr/tiled/none/"), route
    frame.expect(chain(source(t, n_lev), np.where(keep, idx, -1), w.astype(npdt))).check(route)


@pytest.mark.parametrize("t", ["f32", "f64"])
@pytest.mark.parametrize("k", [1, 3, 4])
@pytest.mark.parametrize("n_lev", [1, 3, 137])
def test_field_major_kernel_writes_the_chain_and_nothing_else(dev, n_lev, k, t):
    """lane = target, a store per level inside the level loop (unrolled by 4: 1, 3 and 137 levels leave every remainder); 777 targets
    are three workgroups and a partial one; k = 3 is padded (rows of 1-3 entries)."""
    npdt = DTYPES[t][1]
    idx0, w, lengths = tables()
    padded = k == 3
    idx = np.where(np.arange(4)[None, :] < lengths[:, None], idx0, -1).astype(np.int32)[:, :k] if padded else idx0[:, :k]
    src = np.ascontiguousarray(source(t, n_lev)[:, :n_lev].T)  # (levels, N_SRC)
    frame = Frame(dev, t, n_lev, "fields")
    idx_d, w_d = device_tables(dev, t, k, idx, w)
    native.regrid_ell(torch.from_numpy(src).to(dev).reshape(-1), frame.out, idx_d, w_d, n_src=N_SRC, n_tgt=N_TGT, k=k, n_lev=n_lev, src_pitch=N_SRC,
                      out_pitch=frame.pitch, layout=native.FIELDS, padded=padded)
    route = native.last_gather_route()
    assert route.startswith(f"fields_ell/lanes/none/lane/k{k}/"), route
    frame.expect(np.ascontiguousarray(chain(src.T, idx, None if k == 1 else w[:, :k].astype(npdt)).T)).check(route)


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_what_was_stored_is_what_the_stream_and_the_host_see_next(dev, t):
    """Two launches into the same output, from stack A and then from stack B, a device reduction of the output, a copy of it to the
    host and a per-point kernel that reads it — one stream, nothing in between.  All three show B's result, on whatever XCD they run."""
    n_lev, k = 137, 4
    tdt, npdt, bits = DTYPES[t]
    idx, w, _ = tables()
    pitch = covered(t, n_lev)
    src_a, src_b = (device_source(dev, t, n_lev, seed)[0] for seed in (0, 1))
    idx_d, w_d = device_tables(dev, t, k, idx, w)
    out = torch.empty(N_TGT * pitch, dtype=tdt, device=dev)
    after = torch.empty_like(out)
    prog = native.level_program([[(native.OP_AFFINE, 0, 1.5, -273.25)] * n_lev], dev)
    torch.cuda.synchronize()
    for s in (src_a, src_b):
        native.regrid_ell(s, out, idx_d, w_d, n_src=N_SRC, n_tgt=N_TGT, k=k, n_lev=n_lev, src_pitch=pitch, out_pitch=pitch, layout=native.COLUMNS)
    lo, hi = native.reduce_stack(out, native.RED_MINMAX, n_pts=N_TGT, n_lev=n_lev, pitch=pitch, layout=native.COLUMNS)
    host = out.cpu().numpy().reshape(N_TGT, pitch)
    native.pointwise_stack(out, after, n_pts=N_TGT, n_lev=n_lev, x_pitch=pitch, y_pitch=pitch, layout=native.COLUMNS, prog=prog, n_stage=1)
    rescaled = after.cpu().numpy().reshape(N_TGT, pitch)

    want = chain(source(t, n_lev, 1), idx, w.astype(npdt))
    assert np.array_equal(host.view(bits), want.view(bits)), "the host copy does not hold stack B's result"
    assert (lo, hi) == (float(want[:, :n_lev].min()), float(want[:, :n_lev].max())), "the reduction did not read stack B's result"
    want_after = want[:, :n_lev] * npdt(1.5) + npdt(-273.25)
    assert np.array_equal(rescaled[:, :n_lev].view(bits), want_after.view(bits)), "the per-point kernel did not read stack B's result"
