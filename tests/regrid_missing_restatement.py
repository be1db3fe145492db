"""The missing-value statement of ``atx_regrid_ell_missing`` / ``atx_regrid_csr_missing`` (include/atx_missing.h) restated as plain loops over
numpy scalars of the stack's own type, a second, vectorised formulation of it, and the cases the host and GPU tests share.

For one output element (target t, level l), every operation rounded on its own in T:

    jh = first present entry of row t with the largest weight (strict >); none if the row has no present entry
    for the entries j of row t in table order (index -1: absent, skipped):
        x = src[idx_j, l];  tot = tot + w_j
        x != x:  missing = true;  j == jh: heaviest_missing = true
        else:    num = num + (w_j * x);  den = den + w_j;  n_valid += 1
    not missing                          -> num            (scipy's csr_matvec bits, no division)
    n_valid == 0                         -> NaN
    HEAVIEST and heaviest_missing        -> NaN
    den < T(min_valid) * tot             -> NaN
    else                                 -> num / den

A case holds its table as fixed-k rows (``idx`` [n_tgt, k] with -1 for absent entries, ``w`` [n_tgt, k] in T) and, for CSR cases, the
same rows as (indptr, indices, data); ``src`` is [n_src, n_lev] in T.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

ALL, HEAVIEST = "all", "heaviest"
N_SRC, N_TGT = 300, 131  # the base shape of tests/gather_route_checks.py
NAN_SHARE = (0.0, 1.0, 0.1, 0.3, 0.6, 0.9)  # level l: each source point NaN with probability NAN_SHARE[l % 6]

# the branch an element took
NO_MISSING, ALL_MISSING, HEAVIEST_MISSING, BELOW_MIN_VALID, RENORMALISED = range(5)
BRANCH_NAMES = ("no missing", "all missing", "heaviest missing", "below min_valid", "renormalised")
CONFIGURATIONS = ((ALL, 0.0), (HEAVIEST, 0.0), (ALL, 0.5))


def reachable(policy: str, min_valid: float, k: int) -> tuple:
    """The branches a configuration can reach with rows of k entries."""
    out = [NO_MISSING, ALL_MISSING]
    if k >= 2:
        if policy == HEAVIEST:
            out.append(HEAVIEST_MISSING)
        if min_valid > 0.0:
            out.append(BELOW_MIN_VALID)
        out.append(RENORMALISED)
    return tuple(out)


@dataclass
class MissingCase:
    name: str
    T: type
    k: int
    n_lev: int
    n_src: int
    n_tgt: int
    idx: np.ndarray                        # [n_tgt, k] int32, -1: absent
    w: np.ndarray                          # [n_tgt, k] T (absent entries carry a weight that must not be used)
    src: np.ndarray                        # [n_src, n_lev] T
    padded: bool = False
    csr: Optional[tuple] = None            # (indptr int32 [n_tgt + 1], indices int32 [nnz], data T [nnz]): the same rows
    edges: Optional[dict] = None           # plant_edges: kind -> row

    @property
    def vec(self) -> int:
        return 16 // np.dtype(self.T).itemsize


def bits_type(T):
    return np.uint32 if np.dtype(T).itemsize == 4 else np.uint64


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def restate_element(T, idx_row, w_row, column, policy: str, min_valid: float):
    """One output element: ``column`` is src[:, l].  Returns (value, branch)."""
    zero = T(0)
    jh, best = None, None
    for j in range(len(idx_row)):
        if idx_row[j] < 0:
            continue
        if jh is None or w_row[j] > best:
            jh, best = j, w_row[j]
    num = den = tot = zero
    missing = heaviest_missing = False
    n_valid = 0
    for j in range(len(idx_row)):
        if idx_row[j] < 0:
            continue
        x = column[idx_row[j]]
        wj = w_row[j]
        tot = T(tot + wj)
        if x != x:
            missing = True
            if j == jh:
                heaviest_missing = True
        else:
            num = T(num + T(wj * x))
            den = T(den + wj)
            n_valid += 1
    if not missing:
        return num, NO_MISSING
    if n_valid == 0:
        return T(np.nan), ALL_MISSING
    if policy == HEAVIEST and heaviest_missing:
        return T(np.nan), HEAVIEST_MISSING
    if den < T(T(min_valid) * tot):
        return T(np.nan), BELOW_MIN_VALID
    return T(num / den), RENORMALISED


def restate(case: MissingCase, policy: str, min_valid: float):
    """(out [n_tgt, n_lev] in T, branch [n_tgt, n_lev] int8) by the loops above."""
    assert policy in (ALL, HEAVIEST) and 0.0 <= min_valid <= 1.0
    T = case.T
    out = np.empty((case.n_tgt, case.n_lev), dtype=T)
    branch = np.empty((case.n_tgt, case.n_lev), dtype=np.int8)
    columns = [case.src[:, l] for l in range(case.n_lev)]
    with np.errstate(all="ignore"):
        for t in range(case.n_tgt):
            idx_row, w_row = case.idx[t], case.w[t]
            for l in range(case.n_lev):
                out[t, l], branch[t, l] = restate_element(T, idx_row, w_row, columns[l], policy, min_valid)
    return out, branch


@functools.lru_cache(maxsize=None)
def _restated(key, policy, min_valid):
    return restate(_CASES[key], policy, min_valid)


_CASES: dict = {}


def restated(case: MissingCase, policy: str, min_valid: float):
    """``restate`` computed once per (case, configuration) and shared; the arrays are read-only."""
    _CASES.setdefault(case.name, case)
    assert _CASES[case.name] is case, f"two cases named {case.name}"
    out, branch = _restated(case.name, policy, float(min_valid))
    out.setflags(write=False)
    branch.setflags(write=False)
    return out, branch


def vectorised(case: MissingCase, policy: str, min_valid: float) -> np.ndarray:
    """The same statement as array operations over (target, level), entry by entry — the heaviest entry found up front with argmax."""
    T = case.T
    present = case.idx >= 0
    masked = np.where(present, case.w.astype(np.float64), -np.inf)
    jh = np.where(present.any(axis=1), np.argmax(masked, axis=1), -1)  # argmax: the first among equals
    shape = (case.n_tgt, case.n_lev)
    num, den = np.zeros(shape, dtype=T), np.zeros(shape, dtype=T)
    tot = np.zeros((case.n_tgt, 1), dtype=T)
    missing, heaviest_missing, any_valid = (np.zeros(shape, dtype=bool) for _ in range(3))
    with np.errstate(all="ignore"):
        for j in range(case.k):
            here = present[:, j][:, None]
            wj = case.w[:, j][:, None]
            x = case.src[np.where(present[:, j], case.idx[:, j], 0)]
            nan = np.isnan(x)
            tot = np.where(here, tot + wj, tot).astype(T)
            missing |= here & nan
            heaviest_missing |= here & nan & (jh == j)[:, None]
            use = here & ~nan
            num = np.where(use, num + (wj * x).astype(T), num).astype(T)
            den = np.where(use, den + wj, den).astype(T)
            any_valid |= use
        gone = ~any_valid | (heaviest_missing if policy == HEAVIEST else False) | (den < (T(min_valid) * tot).astype(T))
        return np.where(missing, np.where(gone, T(np.nan), (num / den).astype(T)), num).astype(T)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def special_values(T) -> np.ndarray:
    """One signalling NaN, one NaN with a payload, +-inf, -0.0, a subnormal."""
    if np.dtype(T).itemsize == 4:
        return np.array([0x7FA00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000007], dtype=np.uint32).view(np.float32)
    return np.array([0x7FF4000000000001, 0xFFF8000012345678, 0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000,
                     0x0000000000000007], dtype=np.uint64).view(np.float64)


def make_weights(rng, T, n_tgt: int, k: int) -> np.ndarray:
    """rng.random + 0.05; every 8th row all equal (ties for the heaviest); rows 1::8 one entry exactly 0; rows 2::16 a negative first
    entry (-1/4 of the mean of the others); normalised by row and rounded to T.  (k = 1 keeps its single positive weight.)"""
    w = rng.random((n_tgt, k)) + 0.05
    w[0::8] = w[0::8, :1]
    if k >= 2:
        rows = np.arange(1, n_tgt, 8)
        w[rows, rng.integers(0, k, rows.size)] = 0.0
        w[2::16, 0] = -0.25 * w[2::16, 1:].mean(axis=1)
    if k >= 1:
        w = w / w.sum(axis=1, keepdims=True)
    if k >= 2:
        assert np.all(w[np.arange(1, n_tgt, 8)].min(axis=1) == 0.0)
    return w.astype(T)


def make_sources(rng, T, n_src: int, n_lev: int) -> np.ndarray:
    """280 + 50 N(0, 1); level l NaN with probability NAN_SHARE[l % 6]; the special values planted on valid points."""
    x = (280.0 + 50.0 * rng.standard_normal((n_src, n_lev))).astype(T)
    for l in range(n_lev):
        share = NAN_SHARE[l % 6]
        x[rng.random(n_src) < share, l] = np.nan
        if share == 1.0:
            x[:, l] = np.nan
    valid = np.flatnonzero(~np.isnan(x.reshape(-1)))
    sp = special_values(T)
    if valid.size:
        at = valid[rng.choice(valid.size, size=min(sp.size, valid.size), replace=False)]
        x.reshape(-1).view(bits_type(T))[at] = sp.view(bits_type(T))[: at.size]
    return x


def plant_edges(case: MissingCase) -> None:
    """Edges a random draw meets too rarely, on level 0 (no random NaN there), each in a zero-weight row (1::8) of its own whose sources
    are distinct points no other planted row reads; ``case.edges`` names the rows:
    "inf-under-zero-weight"  +inf under the zero weight — a value, not missing: 0 * inf makes num NaN;
    "nan-under-zero-weight"  NaN under the zero weight only — dropped, and den == tot exactly (the `<` of min_valid = 1);
    "negative-inf"           -inf under a non-zero weight."""
    case.edges = {}
    if case.k < 2:
        return
    T = case.T
    taken: set = set()
    rows = iter(range(1, case.n_tgt, 8))
    for kind, value, under_zero in (("inf-under-zero-weight", np.inf, True), ("nan-under-zero-weight", np.nan, True), ("negative-inf", -np.inf, False)):
        for row in rows:
            slots = [j for j in range(case.k) if case.idx[row, j] >= 0]
            points = [int(case.idx[row, j]) for j in slots]
            pick = [j for j in slots if (case.w[row, j] == 0) == under_zero]
            if len(points) < 2 or len(set(points)) != len(points) or taken & set(points) or not pick:
                continue
            for j in slots:
                case.src[case.idx[row, j], 0] = T(value) if j == pick[0] else T(280.0 + j)
            taken |= set(points)
            case.edges[kind] = row
            break


def make_case(T, k: int, n_lev: int, *, n_src: int = N_SRC, n_tgt: int = N_TGT, padded: bool = False, lengths=None, seed: Optional[int] = None,
              name: Optional[str] = None) -> MissingCase:
    """The case of these arguments, built once and shared (treat it as read-only)."""
    return _make_case(T, k, n_lev, n_src, n_tgt, padded, None if lengths is None else tuple(int(n) for n in lengths), seed, name)


@functools.lru_cache(maxsize=None)
def _make_case(T, k, n_lev, n_src, n_tgt, padded, lengths, seed, name) -> MissingCase:
    """Fixed-k rows (``padded``: ragged, -1 for absent entries anywhere in the row — row 0 all absent, row 1 full, row 2 a single entry
    in the last slot), or CSR rows of ``lengths`` entries (k is then the longest)."""
    tname = "f32" if np.dtype(T).itemsize == 4 else "f64"
    seed = 1000 * k + n_lev if seed is None else seed
    rng = np.random.default_rng(seed)
    if lengths is not None:
        lengths = np.asarray(lengths, dtype=np.int64)
        assert lengths.size == n_tgt
        k = int(lengths.max())
    w = make_weights(rng, T, n_tgt, k)
    idx = rng.integers(0, n_src, (n_tgt, k)).astype(np.int32)
    src = make_sources(rng, T, n_src, n_lev)
    if padded:
        absent = rng.random((n_tgt, k)) < 0.35
        absent[0] = True
        if n_tgt > 1:
            absent[1] = False
        if n_tgt > 2:
            absent[2] = True
            absent[2, k - 1] = False
        idx[absent] = -1
        w[absent] = T(7.0)  # must not be used
    csr = None
    if lengths is not None:
        absent = np.arange(k)[None, :] >= lengths[:, None]
        idx[absent] = -1
        w[absent] = T(7.0)
        indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        csr = (indptr, np.ascontiguousarray(idx[~absent]), np.ascontiguousarray(w[~absent]))
    label = name or f"{tname}-k{k}-L{n_lev}-N{n_tgt}" + ("-padded" if padded else "") + ("-csr" if csr is not None else "") + f"-s{seed}"
    case = MissingCase(label, T, k, n_lev, n_src, n_tgt, idx, w, src, padded=padded, csr=csr)
    plant_edges(case)
    return case


def branch_counts(branch: np.ndarray) -> dict:
    return {b: int(np.count_nonzero(branch == b)) for b in range(5)}
