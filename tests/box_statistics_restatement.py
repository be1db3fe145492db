"""The statement of ``atx_regrid_csr_stat`` (include/atx_stat.h) restated as a plain loop per (target, level) over numpy scalars of the
stack's own type, and the cases the host and GPU tests share.  It shares no code with the package.

For one output element (target t, level l), every operation rounded on its own in T, the entries j of row t in table order:

    w_j = data[j], or T(1) where data is None
    jh  = the first entry of the row with the largest w (strict >)
    for every entry:  tot = tot + w_j;  x_j = src[indices[j], l]
        x_j != x_j : missing = true;  j == jh: heaviest_missing = true
        else       : j is VALID;  den = den + w_j
    out = NaN  when the row has no valid entry (an empty row included)
        = NaN  under ANY when missing;  under HEAVIEST when heaviest_missing
        = NaN  when den < T(min_valid) * tot
    otherwise, over the valid entries in row order:
      maximum   m = first valid x;  then  m = (x_j > m) ? x_j : m
      minimum   the same with <
      mode      W_j = sum from T(0), in row order, of w_i over valid i with x_i == x_j
                best = first valid j;  a later j replaces it when  W_j > W_best,  or  W_j == W_best and x_j < x_best;  out = x_best
      variance  num = sum (w_j * x_j);  mean = num / den;  d_j = x_j - mean;  s = sum (w_j * (d_j * d_j));  out = s / den
      standard-deviation   sqrt(variance), correctly rounded

``restate_element(..., defect=)`` plants one of ``DEFECTS`` — a wrong reading of the statement that the host tests must notice.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

ANY, ALL, HEAVIEST = None, "all", "heaviest"
MAXIMUM, MINIMUM, MODE, VARIANCE, STDDEV = "maximum", "minimum", "mode", "variance", "standard-deviation"
STATISTICS = (MAXIMUM, MINIMUM, MODE, VARIANCE, STDDEV)
# (policy, min_valid): every policy with min_valid 0, 0.5 and 1 among them
CONFIGS = ((ANY, 0.0), (ALL, 0.0), (HEAVIEST, 0.0), (ALL, 0.5), (HEAVIEST, 1.0), (ANY, 0.5), (ALL, 1.0), (HEAVIEST, 0.5), (ANY, 1.0))
ROW_LENGTHS = [0, 70, 1, 4, 5, 0] + [3, 0, 5, 2, 9] * 25  # test_csr_rows of the missing-value suite
N_SRC = 300
NAN_SHARE = (0.0, 1.0, 0.1, 0.3, 0.6, 0.9)  # level l: each source point NaN with probability NAN_SHARE[l % 6]
DEFECTS = ("tie-rule-ge", "mode-ignores-weights", "nan-counted-valid", "tot-for-den", "second-pass-skipped")


def bits_type(T):
    return np.uint32 if np.dtype(T).itemsize == 4 else np.uint64


@dataclass
class StatCase:
    name: str
    T: type
    n_src: int
    n_tgt: int
    n_lev: int
    indptr: np.ndarray             # [n_tgt + 1] int32
    indices: np.ndarray            # [nnz] int32
    data: Optional[np.ndarray]     # [nnz] T, or None: every entry weighs 1
    src: np.ndarray                # [n_src, n_lev] T

    @property
    def vec(self) -> int:
        return 16 // np.dtype(self.T).itemsize


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def restate_element(T, idx_row, w_row, column, statistic, policy, min_valid, defect=None):
    """One output element: ``idx_row`` / ``w_row`` are the row's entries (``w_row`` of T scalars), ``column`` is src[:, l]."""
    zero, nan = T(0), T(np.nan)
    n = len(idx_row)
    jh, best = None, None
    for j in range(n):
        if jh is None or w_row[j] > best:
            jh, best = j, w_row[j]
    tot = den = zero
    missing = heaviest_missing = False
    valid = []
    for j in range(n):
        x = column[idx_row[j]]
        tot = T(tot + w_row[j])
        if x != x and defect != "nan-counted-valid":
            missing = True
            if j == jh:
                heaviest_missing = True
        else:
            valid.append(j)
            den = T(den + w_row[j])
    if not valid:
        return nan
    if (policy is ANY and missing) or (policy == HEAVIEST and heaviest_missing):
        return nan
    if den < T(T(min_valid) * tot):
        return nan
    xs = [column[idx_row[j]] for j in valid]
    ws = [w_row[j] for j in valid]
    if statistic in (MAXIMUM, MINIMUM):
        m = xs[0]
        for x in xs[1:]:
            if (x > m) if statistic == MAXIMUM else (x < m):
                m = x
        return m
    if statistic == MODE:
        W = []
        for a in range(len(xs)):
            acc = zero
            for b in range(len(xs)):
                if xs[b] == xs[a]:
                    acc = T(acc + (T(1) if defect == "mode-ignores-weights" else ws[b]))
            W.append(acc)
        b = 0
        for a in range(1, len(xs)):
            if defect == "tie-rule-ge":
                better = W[a] >= W[b]
            else:
                better = W[a] > W[b] or (W[a] == W[b] and xs[a] < xs[b])
            if better:
                b = a
        return xs[b]
    assert statistic in (VARIANCE, STDDEV), statistic
    over = tot if defect == "tot-for-den" else den
    num = zero
    for x, w in zip(xs, ws):
        num = T(num + T(w * x))
    mean = zero if defect == "second-pass-skipped" else T(num / over)
    s = zero
    for x, w in zip(xs, ws):
        d = T(x - mean)
        s = T(s + T(w * T(d * d)))
    var = T(s / over)
    return var if statistic == VARIANCE else T(np.sqrt(var))


def restate(case: StatCase, statistic, policy, min_valid: float, defect=None) -> np.ndarray:
    """out [n_tgt, n_lev] in T by the loop above."""
    assert statistic in STATISTICS and policy in (ANY, ALL, HEAVIEST) and 0.0 <= min_valid <= 1.0
    T = case.T
    out = np.empty((case.n_tgt, case.n_lev), dtype=T)
    columns = [case.src[:, l] for l in range(case.n_lev)]
    with np.errstate(all="ignore"):
        for t in range(case.n_tgt):
            lo, hi = int(case.indptr[t]), int(case.indptr[t + 1])
            idx_row = case.indices[lo:hi]
            w_row = [T(1)] * (hi - lo) if case.data is None else list(case.data[lo:hi])
            for l in range(case.n_lev):
                out[t, l] = restate_element(T, idx_row, w_row, columns[l], statistic, policy, min_valid, defect)
    return out


_CASES: dict = {}


@functools.lru_cache(maxsize=None)
def _restated(key, statistic, policy, min_valid):
    return restate(_CASES[key], statistic, policy, min_valid)


def restated(case: StatCase, statistic, policy, min_valid: float) -> np.ndarray:
    """``restate`` computed once per (case, configuration) and shared; the array is read-only."""
    _CASES.setdefault(case.name, case)
    assert _CASES[case.name] is case, f"two cases named {case.name}"
    out = _restated(case.name, statistic, policy, float(min_valid))
    out.setflags(write=False)
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def special_values(T) -> np.ndarray:
    """One signalling NaN, one NaN with a payload, +-inf, -0.0, a subnormal."""
    if np.dtype(T).itemsize == 4:
        return np.array([0x7FA00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000007], dtype=np.uint32).view(np.float32)
    return np.array([0x7FF4000000000001, 0xFFF8000012345678, 0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000,
                     0x0000000000000007], dtype=np.uint64).view(np.float64)


def make_sources(rng, T, n_src: int, n_lev: int, categorical: bool) -> np.ndarray:
    """Continuous: 280 + 50 N(0, 1), the special values planted on valid points.  Categorical: the integers 0 .. 5 (rows of 2 - 9 entries
    then hold repeated classes and ties).  Level l is NaN with probability NAN_SHARE[l % 6]."""
    if categorical:
        x = rng.integers(0, 6, (n_src, n_lev)).astype(T)
    else:
        x = (280.0 + 50.0 * rng.standard_normal((n_src, n_lev))).astype(T)
    for l in range(n_lev):
        share = NAN_SHARE[l % 6]
        x[rng.random(n_src) < share, l] = np.nan
        if share == 1.0:
            x[:, l] = np.nan
    if not categorical:
        valid = np.flatnonzero(~np.isnan(x.reshape(-1)))
        sp = special_values(T)
        if valid.size:
            at = valid[rng.choice(valid.size, size=min(sp.size, valid.size), replace=False)]
            x.reshape(-1).view(bits_type(T))[at] = sp.view(bits_type(T))[: at.size]
    return x


def make_weights(rng, T, lengths: np.ndarray) -> np.ndarray:
    """Shares of a cell: rng.random + 0.05 normalised by row and rounded to T; every 4th row all equal (ties for the heaviest entry and
    between classes); rows 1::8 one entry exactly 0."""
    parts = []
    for t, n in enumerate(lengths):
        w = rng.random(n) + 0.05
        if t % 4 == 0:
            w[:] = 0.25
        elif t % 8 == 1 and n >= 2:
            w[rng.integers(0, n)] = 0.0
        if n and t % 4:
            w = w / w.sum()
        parts.append(w)
    return np.concatenate(parts).astype(T) if parts else np.zeros(0, dtype=T)


def make_case(T, n_lev: int, *, lengths=None, n_tgt: Optional[int] = None, n_src: int = N_SRC, categorical: bool = False, weighted: bool = True,
              seed: Optional[int] = None, name: Optional[str] = None) -> StatCase:
    """The case of these arguments, built once and shared (treat it as read-only).  ``lengths``: the row lengths (default ROW_LENGTHS,
    or its first ``n_tgt``, repeated as needed)."""
    if lengths is None:
        lengths = ROW_LENGTHS
        if n_tgt is not None:
            lengths = (ROW_LENGTHS[1:] * (n_tgt // len(ROW_LENGTHS) + 2))[:n_tgt]  # (starts with the row of 70)
    return _make_case(T, n_lev, tuple(int(n) for n in lengths), n_src, categorical, weighted, seed, name)


@functools.lru_cache(maxsize=None)
def _make_case(T, n_lev, lengths, n_src, categorical, weighted, seed, name) -> StatCase:
    tname = "f32" if np.dtype(T).itemsize == 4 else "f64"
    lengths = np.asarray(lengths, dtype=np.int64)
    n_tgt = lengths.size
    seed = 7000 + 10 * n_lev + n_tgt if seed is None else seed
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = rng.integers(0, n_src, int(indptr[-1])).astype(np.int32)
    data = make_weights(rng, T, lengths) if weighted else None
    src = make_sources(rng, T, n_src, n_lev, categorical)
    label = name or f"{tname}-L{n_lev}-N{n_tgt}-nnz{int(indptr[-1])}" + ("-cat" if categorical else "") + ("" if weighted else "-unweighted") + f"-s{seed}"
    return StatCase(label, T, n_src, n_tgt, n_lev, indptr, indices, data, src)


def rows_case(T, name: str, rows, weights=None) -> StatCase:
    """A single-level case whose row t reads the values ``rows[t]`` (each value a source point of its own) with the weights
    ``weights[t]`` (default: all 0.25)."""
    lengths = [len(r) for r in rows]
    flat = np.array([v for r in rows for v in r], dtype=T)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = np.arange(flat.size, dtype=np.int32)
    data = np.full(flat.size, 0.25, dtype=T) if weights is None else np.array([w for r in weights for w in r], dtype=T)
    assert data.size == flat.size
    src = np.concatenate([flat, np.zeros(1, dtype=T)]).reshape(-1, 1)  # (never empty)
    return StatCase(name, T, src.shape[0], len(rows), 1, indptr, indices, data, src)


def same(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Element by element: the bits where ``want`` is a number, a NaN where it is one."""
    B = bits_type(want.dtype.type)
    return np.where(np.isnan(want), np.isnan(got), got.view(B) == want.view(B))
