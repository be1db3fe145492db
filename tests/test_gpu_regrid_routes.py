"""Every instantiation the fixed-k dispatch ladders can reach, and the direct kernel's workgroup-to-XCD stripes.

The ladders of the gather (csrc/atx_regrid_columns.inc, atx_regrid_fields.inc) pick a compile-time k — columns 1..8, 12, 16,
padded columns 3..8, 12, 16, fields 1..4, padded fields 3, 4 — and send everything else to a runtime-k loop; `set_tuning(tile > 0)`
moves a column stack from the direct kernel to the tiled one.  Each of these is run here on a shape small enough for a few
milliseconds and awkward enough to go wrong: 131 targets of 5 levels are 2 / 3 sixteen-byte vectors per column with a partial last
one, two workgroups with a tail, and no tile size divides 131.  The bar is `assert_interp`'s: scipy's csr_matvec in the stack's
own width, bit for bit in float32 and float64.  Outputs start as NaN so that a row nobody visited shows.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from anemoi_transform_amd import native
from anemoi_transform_amd.stack import COLUMNS, Stack
from oracle import oracle
from test_gpu_kernels import DTYPES, LAYOUTS, assert_interp, make_fields, random_ell, to_dev

pytestmark = pytest.mark.gpu

N_SRC, N_TGT, N_LEV = 300, 131, 5
LADDER_K = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16]  # compile-time k of the column ladder (the field ladder stops at 4)
RUNTIME_K = [9, 11, 17]
# (k, padded, weighted): every k with weights — k = 1 too, or the ladders' `case 1` is never reached — and the pure gather, which the
# dispatch takes before the ladder (w == NULL)
CASES = ([(k, False, True) for k in LADDER_K + RUNTIME_K] + [(k, True, True) for k in LADDER_K + RUNTIME_K if k >= 3] + [(1, False, False)])


def padded_table(rng, idx, w):
    """Rows of 0..k present entries, the absent ones (-1, weight 0) anywhere in the row — the first entry included: atx.h lets
    any entry be absent and gives a row of only absent entries 0, as scipy does."""
    n_tgt, k = idx.shape
    lengths = rng.integers(0, k + 1, size=n_tgt)
    lengths[:3] = (0, k, 1)  # an empty row, a full one and a single entry, whatever the draw
    present = np.stack([rng.permutation(k) < n for n in lengths])
    present[2] = np.arange(k) == k - 1  # the single entry last: the row's first entry is absent
    return np.where(present, idx, -1).astype(np.int32), np.where(present, w, 0).astype(w.dtype)


def csr_of(idx, w):
    present = idx >= 0
    indptr = np.concatenate([[0], np.cumsum(present.sum(axis=1))])
    return w[present], idx[present], indptr


@functools.lru_cache(maxsize=None)
def ladder_case(k, padded, np_dtype, n_lev):
    """Tables, two source field sets and scipy's answer for each: computed once, shared by both layouts; nobody writes to them."""
    rng = np.random.default_rng(1000 * k + 10 * n_lev + padded)
    xs = [make_fields(rng, n_lev, N_SRC, np_dtype) for _ in range(2)]
    idx, w = random_ell(rng, N_SRC, N_TGT, k, np_dtype)
    if padded:
        idx, w = padded_table(rng, idx, w)
    data, indices, indptr = csr_of(idx, w)
    wants = [np.stack([oracle.csr_apply(data, indices, indptr, (N_TGT, N_SRC), f) for f in x]) for x in xs]
    order = rng.permutation(N_TGT).astype(np.int32)
    return xs, idx, w, wants, order


def run_ladder(dev, k, padded, weighted, np_dtype, layout, n_lev):
    """`weighted` False (k = 1 only): no weight table, the pure gather; random_ell's single weight is 1.0, so scipy's row sum
    0 + 1.0 * x has the same bits either way."""
    xs, idx, w, wants, order = ladder_case(k, padded, np_dtype, n_lev)
    srcs = [Stack.from_fields(x, dev=dev, layout=layout) for x in xs]
    tables = [(to_dev(idx, dev), to_dev(w, dev) if weighted else None, None)]
    if layout == COLUMNS:  # the ordered entry point: table row t is output row order[t]
        tables.append((to_dev(idx[order], dev), to_dev(w[order], dev) if weighted else None, to_dev(order, dev)))
    for tile in (0, 8):  # the direct kernel, and the tiled one
        for idx_d, w_d, rows in tables:
            for n_stack in (1, 2):
                outs = [srcs[0].new_like(n_pts=N_TGT) for _ in range(n_stack)]
                for o in outs:
                    o.data.fill_(float("nan"))
                native.set_tuning(tile)
                try:
                    native.regrid_ell_batch([s.data for s in srcs[:n_stack]], [o.data for o in outs], idx_d, w_d, n_src=N_SRC, n_tgt=N_TGT,
                                            k=k, n_lev=n_lev, src_pitch=srcs[0].pitch, out_pitch=outs[0].pitch, layout=layout,
                                            padded=padded, tgt_rows=rows)
                finally:
                    native.set_tuning(0)
                for o, want in zip(outs, wants):
                    assert_interp(o.numpy(), want, np_dtype)


@pytest.mark.parametrize("tdtype,np_dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,padded,weighted", CASES)
def test_every_ladder_instantiation_gives_scipys_bits(dev, tdtype, np_dtype, layout, k, padded, weighted):
    """Compile-time and runtime k, plain and padded, direct and tiled kernel, natural and ordered traversal, one stack and two."""
    run_ladder(dev, k, padded, weighted, np_dtype, layout, N_LEV)


@pytest.mark.parametrize("tdtype,np_dtype", DTYPES)
@pytest.mark.parametrize("padded", [False, True])
def test_one_level_column_stack_takes_the_scalar_instantiation(dev, tdtype, np_dtype, padded):
    """A one-level column stack is stored tight (stack.column_pitch): no 16-byte vectors, the VEC = 1 instantiations, k = 4."""
    assert Stack.empty(N_TGT, 1, tdtype, dev, COLUMNS).pitch == 1
    run_ladder(dev, 4, padded, True, np_dtype, COLUMNS, 1)


@pytest.mark.parametrize("k", [5, 16])
@pytest.mark.parametrize("n_tgt", [511 * 256, 512 * 256, 512 * 256 + 1, 1024 * 256 + 300])
def test_direct_kernel_stripes_cover_every_row(dev, k, n_tgt):
    """Rows of 5 entries or more in natural order have the direct kernel's workgroups dealt to the 8 XCDs in stripes of 64
    (xcd_stripe), which permutes only from 8 x 64 = 512 workgroups of 256 items.  A tight one-level float64 column stack is one item
    per target: below one group of stripes, exactly one, a tail of one workgroup, two groups and a partial tail — every row is
    computed once, with scipy's bits, and the ordered entry point (contiguous ranges, xcd_tile) with the identity order agrees."""
    rng = np.random.default_rng(k * n_tgt)
    n_src = 1000
    x = make_fields(rng, 1, n_src, np.float64)
    idx, w = random_ell(rng, n_src, n_tgt, k, np.float64)
    want = oracle.csr_apply(w.reshape(-1), idx.reshape(-1), np.arange(n_tgt + 1) * k, (n_tgt, n_src), x[0])[None]
    src = Stack.from_fields(x, dev=dev, layout=COLUMNS)
    assert src.pitch == 1
    idx_d, w_d = to_dev(idx, dev), to_dev(w, dev)
    identity = torch.arange(n_tgt, dtype=torch.int32, device=dev)
    for rows in (None, identity):
        out = src.new_like(n_pts=n_tgt)
        out.data.fill_(float("nan"))
        native.regrid_ell(src.data, out.data, idx_d, w_d, n_src=n_src, n_tgt=n_tgt, k=k, n_lev=1, src_pitch=src.pitch,
                          out_pitch=out.pitch, layout=COLUMNS, tgt_rows=rows)
        assert_interp(out.numpy(), want, np.float64)
