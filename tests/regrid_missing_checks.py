"""The checks that hold ``regrid_ell_missing`` / ``regrid_csr_missing`` to the restatement (tests/regrid_missing_restatement.py) — plain
functions over the callables under test.  tests/test_gpu_regrid_missing.py runs them on ``native.*`` on an MI355X;
tests/test_regrid_missing_host.py runs them on the CPU against a numpy stand-in that walks the buffers as the kernels do, once as it is
and once per planted defect.

``check_case`` lays a case out in pitched buffers of one of the ``FORMS``, runs one configuration and asserts, no element left out:
- every element whose restated value is a number has its bits, every other one is a NaN;
- the output allocation starts as a canary pattern: the guard rows before and after the stack keep it, and so does the pitch padding —
  all of it on the scalar form, everything beyond the 16-byte vector that holds the last level on the vector form;
- the form is the one the case is written for (restated from the addresses and pitches, as the launcher decides it);
- sources and tables are unchanged afterwards.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import numpy as np

from regrid_missing_restatement import BRANCH_NAMES, MissingCase, bits_type, restated

COLUMNS = 0
GUARD_ROWS = 2
FORMS = ("tight", "loose", "odd-pitch", "offset")  # the first two take 16-byte vectors, the last two single elements


@dataclass
class Kernels:
    """The callables under test — ``native_missing.regrid_ell_missing`` / ``native_missing.regrid_csr_missing`` or a stand-in with their signatures —
    and how a host array becomes a buffer they take."""

    regrid_ell_missing: Callable
    regrid_csr_missing: Callable
    upload: Callable    # numpy array (1-D) -> buffer
    download: Callable  # buffer -> numpy array
    address: Callable   # buffer -> address of its first element


def canary(T, n: int) -> np.ndarray:
    bits = np.full(n, 0xC0DEC0DE if np.dtype(T).itemsize == 4 else 0xC0DEC0DEC0DEC0DE, dtype=bits_type(T))
    return bits.view(T)


def aligned_empty(T, n: int) -> np.ndarray:
    """n elements of T whose first one sits on a 16-byte boundary."""
    size = np.dtype(T).itemsize
    raw = np.empty(n * size + 16, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 16
    return raw[skip: skip + n * size].view(T)


def pitches(case: MissingCase, form: str) -> tuple:
    """(src_pitch, out_pitch, offset of both bases in elements) of a form."""
    v = case.vec
    covered = -(-case.n_lev // v) * v
    if form == "tight":
        return covered, covered, 0
    if form == "loose":
        return covered + 2 * v, covered + v, 0
    if form == "odd-pitch":
        assert (case.n_lev + 1) % v != 0, "n_lev + 1 is a whole number of vectors: choose another n_lev for the scalar form"
        return case.n_lev + 1, case.n_lev + 1, 0
    assert form == "offset"
    return covered, covered, 1


def vector_form(T, addresses, n_lev: int, sp: int, op: int) -> bool:
    """The launcher's condition: 16-byte bases and pitches, the last (partial) vector inside both pitches."""
    v = 16 // np.dtype(T).itemsize
    covered = -(-n_lev // v) * v
    return all(a % 16 == 0 for a in addresses) and sp % v == 0 and op % v == 0 and covered <= sp and covered <= op


def first_difference(case, got, want, branch) -> str:
    B = bits_type(case.T)
    nan_w = np.isnan(want)
    bad = np.where(nan_w, ~np.isnan(got), got.view(B) != want.view(B))
    t, l = (int(a[0]) for a in np.nonzero(bad))
    return (f"{int(bad.sum())} of {bad.size} elements differ; first at target {t}, level {l} ({BRANCH_NAMES[branch[t, l]]}): got {got[t, l]!r} "
            f"(bits {int(got.view(B)[t, l]):#x}), want {want[t, l]!r} (bits {int(want.view(B)[t, l]):#x}); row idx {case.idx[t].tolist()}, "
            f"w {case.w[t].tolist()}, sources {[None if i < 0 else case.src[i, l] for i in case.idx[t]]}")


def check_case(kern: Kernels, case: MissingCase, policy: str, min_valid: float, form: str = "tight", table: str = "ell") -> None:
    T = case.T
    B = bits_type(T)
    what = f"{case.name} {policy} min_valid={min_valid} {form} {table}"
    sp, op, off = pitches(case, form)
    # sources: canary in the padding
    src_host = aligned_empty(T, off + case.n_src * sp)
    src_host[:] = canary(T, src_host.size)
    src_rows = src_host[off:].reshape(case.n_src, sp)
    src_rows[:, : case.n_lev] = case.src
    # output: guard rows before and after
    n_rows = GUARD_ROWS + case.n_tgt + GUARD_ROWS
    out_host = aligned_empty(T, off + n_rows * op)
    out_host[:] = canary(T, out_host.size)
    src_d, out_d = kern.upload(src_host), kern.upload(out_host)
    src_base = src_d[off:]
    out_base = out_d[off + GUARD_ROWS * op:]
    vector = vector_form(T, (kern.address(src_base), kern.address(out_base)), case.n_lev, sp, op)
    assert vector == (form in ("tight", "loose")), f"{what}: the case is written for the {'vector' if form in ('tight', 'loose') else 'scalar'} form"
    common = dict(n_src=case.n_src, n_tgt=case.n_tgt, n_lev=case.n_lev, src_pitch=sp, out_pitch=op, layout=COLUMNS, policy=policy,
                  min_valid=min_valid)
    if table == "ell":
        tables_host = (np.ascontiguousarray(case.idx.reshape(-1)), np.ascontiguousarray(case.w.reshape(-1)))
        tables = tuple(kern.upload(a.copy()) for a in tables_host)
        kern.regrid_ell_missing(src_base, out_base, tables[0], tables[1], k=case.k, padded=case.padded, **common)
    else:
        indptr, indices, data = case.csr
        tables_host = (indptr, indices, data)
        tables = tuple(kern.upload(a.copy()) for a in tables_host)
        kern.regrid_csr_missing(src_base, out_base, tables[0], tables[1], tables[2], nnz=len(indices), **common)
    after = kern.download(out_d)
    want, branch = restated(case, policy, min_valid)
    rows = after[off:].reshape(n_rows, op)
    got = np.ascontiguousarray(rows[GUARD_ROWS: GUARD_ROWS + case.n_tgt, : case.n_lev])
    nan_w = np.isnan(want)
    same = np.where(nan_w, np.isnan(got), got.view(B) == want.view(B))
    assert same.all(), f"{what}: {first_difference(case, got, want, branch)}"
    # what must not be written
    can = canary(T, 1).view(B)[0]
    assert (after[:off].view(B) == can).all(), f"{what}: elements before the base written"
    assert (rows[:GUARD_ROWS].view(B) == can).all(), f"{what}: rows before the stack written"
    assert (rows[GUARD_ROWS + case.n_tgt:].view(B) == can).all(), f"{what}: rows after the stack written"
    written_to = -(-case.n_lev // case.vec) * case.vec if vector else case.n_lev
    assert (rows[GUARD_ROWS: GUARD_ROWS + case.n_tgt, written_to:].view(B) == can).all(), f"{what}: pitch padding beyond element {written_to} written"
    # inputs unchanged
    assert (kern.download(src_d).view(B) == src_host.view(B)).all(), f"{what}: sources changed"
    for name, a, d in zip(("first", "second", "third"), tables_host, tables):
        assert np.array_equal(kern.download(d).view(np.uint8), a.view(np.uint8)), f"{what}: the {name} table changed"
