"""Missing-value-aware regridding without a GPU: the restatement against scipy's product and a second formulation, the coverage of its
branches, the checks of tests/regrid_missing_checks.py against a numpy stand-in that walks the buffers as the kernels do — once as it is
and once per planted defect —, the argument validation of the two entry points, and the Python layers above them."""

from __future__ import annotations

import ctypes
import logging

import numpy as np
import pytest

from anemoi_transform_amd import native, native_missing
from anemoi_transform_amd.filters import create_filter_by_name, fusion
from anemoi_transform_amd.gather import GatherPlan
from oracle import oracle

import regrid_missing_restatement as rs
from regrid_missing_checks import Kernels, check_case, vector_form

COVERAGE_K = (2, 3, 4, 8, 16, 17)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_restatement_is_scipys_product_on_complete_stacks(T):
    """Without a NaN among the sources every element is csr_matvec's, bit for bit: the num loop IS csr_matvec's loop."""
    for k in range(1, 18):
        case = rs.make_case(T, k, 3, n_tgt=40, seed=77 + k, name=f"complete-{T.__name__}-k{k}")
        case.src[:] = (280.0 + 50.0 * np.random.default_rng(k).standard_normal(case.src.shape)).astype(T)
        indptr = np.arange(case.n_tgt + 1) * k
        for policy, min_valid in ((rs.ALL, 0.0), (rs.HEAVIEST, 1.0)):
            got, branch = rs.restate(case, policy, min_valid)
            assert (branch == rs.NO_MISSING).all()
            for l in range(case.n_lev):
                want = oracle.csr_apply(case.w.reshape(-1), case.idx.reshape(-1), indptr, (case.n_tgt, case.n_src), np.ascontiguousarray(case.src[:, l]))
                assert want.dtype == T and np.array_equal(got[:, l].view(rs.bits_type(T)), want.view(rs.bits_type(T))), (k, l, policy)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_restatement_equals_the_vectorised_formulation(T):
    B = rs.bits_type(T)
    cases = [rs.make_case(T, k, 7, n_tgt=67) for k in (1, 2, 4, 5, 17)]
    cases.append(rs.make_case(T, 6, 7, n_tgt=67, padded=True))
    cases.append(rs.make_case(T, 0, 7, n_tgt=67, lengths=[0, 9, 1] + [3, 0, 5, 2] * 16))
    for case in cases:
        for policy, min_valid in rs.CONFIGURATIONS + ((rs.HEAVIEST, 1.0),):
            want, _ = rs.restated(case, policy, min_valid)
            got = rs.vectorised(case, policy, min_valid)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(B)[~nan], want.view(B)[~nan]), (case.name, policy, min_valid)


def test_every_reachable_branch_is_well_covered():
    """At 25 levels each branch a configuration can reach holds at least 250 of the 131 x 25 = 3275 elements, for every k of the sweep
    (seeds 1000 k + n_lev); k = 1 has only the first two."""
    for k in COVERAGE_K + (1,):
        case = rs.make_case(np.float32, k, 25)
        for policy, min_valid in rs.CONFIGURATIONS:
            _, branch = rs.restated(case, policy, min_valid)
            counts = rs.branch_counts(branch)
            assert branch.size == 3275
            can = rs.reachable(policy, min_valid, k)
            for b in range(5):
                if b in can:
                    assert counts[b] >= 250, (k, policy, min_valid, rs.BRANCH_NAMES[b], counts)
                elif b != rs.BELOW_MIN_VALID:  # (with min_valid = 0 a negative sum of valid weights lands there: the rows 2::16)
                    assert counts[b] == 0, (k, policy, min_valid, rs.BRANCH_NAMES[b], counts)


def test_the_planted_edges_are_there():
    """+inf under a zero weight makes num NaN without being missing; a NaN under a zero weight alone leaves den == tot."""
    case = rs.make_case(np.float64, 4, 5)
    out, branch = rs.restated(case, rs.ALL, 1.0)
    assert sorted(case.edges) == ["inf-under-zero-weight", "nan-under-zero-weight", "negative-inf"]
    row = case.edges["inf-under-zero-weight"]
    assert branch[row, 0] == rs.NO_MISSING and np.isnan(out[row, 0])
    row = case.edges["nan-under-zero-weight"]
    assert branch[row, 0] == rs.RENORMALISED and np.isfinite(out[row, 0])
    row = case.edges["negative-inf"]
    assert branch[row, 0] == rs.NO_MISSING and out[row, 0] == -np.inf
    for k in (2, 4, 5, 8, 17):  # every case of the check lists has the two zero-weight edges
        assert {"inf-under-zero-weight", "nan-under-zero-weight"} <= set(rs.make_case(np.float32, k, 5, n_tgt=67).edges), k


# ---- a stand-in that walks the buffers as the kernels do -----------------------------------------------------------------------------
DEFECTS = ("divides-when-nothing-is-missing", "fused-multiply-add", "last-among-equal-weights-is-heaviest", "nan-tested-on-the-product",
           "le-for-lt-at-min-valid", "absent-entry-counted-in-tot", "zero-weight-nan-propagates", "heaviest-chosen-per-level-among-valid")
LADDER = (1, 2, 3, 4, 8, 16)  # csrc/missing/atx_regrid_missing.hip: launch_ell_missing
STEP = 4                      # kMissingStep


class StandIn:
    """One (target, vector) item per lane: the row walked once, STEP entries at a time, a running largest weight per row and num, den
    and three flags per element; stores of whole vectors.  Every read and write is checked against its buffer."""

    def __init__(self, defect: str | None = None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    def regrid_ell_missing(self, src, out, idx, w, *, n_src, n_tgt, k, n_lev, src_pitch, out_pitch, layout, policy, min_valid, padded=False):
        assert layout == 0 and w is not None and 1 <= k <= 64
        start = np.arange(n_tgt, dtype=np.int64) * k
        self._walk(src, out, idx, w, start, np.full(n_tgt, k, dtype=np.int64), k if k in LADDER else STEP, n_src, n_tgt, n_lev, src_pitch, out_pitch,
                   policy, min_valid)

    def regrid_csr_missing(self, src, out, indptr, indices, data, *, n_src, n_tgt, nnz, n_lev, src_pitch, out_pitch, layout, policy, min_valid):
        assert layout == 0 and len(indices) == nnz
        start = indptr[:-1].astype(np.int64)
        self._walk(src, out, indices, data, start, np.diff(indptr.astype(np.int64)), STEP, n_src, n_tgt, n_lev, src_pitch, out_pitch, policy, min_valid)

    def _walk(self, src, out, ip, wp, start, length, step, n_src, n_tgt, n_lev, sp, op, policy, min_valid):
        T = src.dtype.type
        defect = self.defect
        vec = 16 // src.dtype.itemsize if vector_form(T, (src.ctypes.data, out.ctypes.data), n_lev, sp, op) else 1
        C = -(-n_lev // vec)
        q = np.arange(n_tgt * C, dtype=np.int64)
        t, c = q // C, q % C
        lanes = np.arange(vec)
        num, den = np.zeros((q.size, vec), dtype=T), np.zeros((q.size, vec), dtype=T)
        missing, valid, heaviest_missing = (np.zeros((q.size, vec), dtype=bool) for _ in range(3))
        tot, best, have = np.zeros(q.size, dtype=T), np.zeros(q.size, dtype=T), np.zeros(q.size, dtype=bool)
        best_valid, have_valid = np.zeros((q.size, vec), dtype=T), np.zeros((q.size, vec), dtype=bool)  # (one defect's own state)
        n_steps = -(-int(length.max()) // step) if q.size else 0
        spare = np.zeros(q.size, dtype=np.int64)
        wide = np.float64 if T is np.float32 else np.longdouble
        with np.errstate(all="ignore"):
            for j in range(n_steps * step):
                inside = j < length[t]
                at = np.where(inside, start[t] + j, 0)
                assert at.size == 0 or (at.min() >= 0 and at.max() < max(len(ip), 1))
                p = np.where(inside, ip[at] if len(ip) else 0, -1).astype(np.int64)
                wj = np.where(inside, wp[at] if len(wp) else 0, 0).astype(T)
                if j == 0:
                    spare = np.where(p >= 0, p, 0)
                row = np.where(p >= 0, p, spare)
                assert (row >= 0).all() and (row < n_src).all()
                address = row * sp + c * vec
                assert (address + vec <= src.size).all(), "a source read past the allocation"
                x = src[address[:, None] + lanes]
                present = p >= 0
                counted = inside if defect == "absent-entry-counted-in-tot" else present
                tot = np.where(counted, tot + wj, tot).astype(T)
                heavier = present & (~have | ((wj >= best) if defect == "last-among-equal-weights-is-heaviest" else (wj > best)))
                best = np.where(heavier, wj, best)
                have |= present
                prod = (wj[:, None] * x).astype(T)
                nan = np.isnan(prod) if defect == "nan-tested-on-the-product" else np.isnan(x)
                if defect == "zero-weight-nan-propagates":
                    nan = nan & (wj != 0)[:, None]
                use = present[:, None] & ~nan
                if defect == "fused-multiply-add":
                    summed = (wj[:, None].astype(wide) * x.astype(wide) + num.astype(wide)).astype(T)
                else:
                    summed = (num + prod).astype(T)
                num = np.where(use, summed, num)
                den = np.where(use, (den + wj[:, None]).astype(T), den)
                missing |= present[:, None] & nan
                valid |= use
                if defect == "heaviest-chosen-per-level-among-valid":
                    better = use & (~have_valid | (wj[:, None] > best_valid))
                    best_valid = np.where(better, wj[:, None], best_valid)
                    have_valid |= use
                    heaviest_missing = np.where(better, False, heaviest_missing)
                else:
                    heaviest_missing = np.where(heavier[:, None], nan, heaviest_missing)
            need = (T(min_valid) * tot).astype(T)[:, None]
            short = (den <= need) if defect == "le-for-lt-at-min-valid" else (den < need)
            gone = ~valid | ((policy == rs.HEAVIEST) & heaviest_missing) | short
            quotient = (num / den).astype(T)
            result = np.where(missing, np.where(gone, T(np.nan), quotient), quotient if defect == "divides-when-nothing-is-missing" else num).astype(T)
        address = t * op + c * vec
        assert q.size == 0 or (address.min() >= 0 and (address + vec <= out.size).all()), "a store past the allocation"
        out[address[:, None] + lanes] = result


def stand_in(defect=None) -> Kernels:
    double = StandIn(defect)
    return Kernels(double.regrid_ell_missing, double.regrid_csr_missing, upload=lambda a: a, download=lambda a: a.copy(), address=lambda a: a.ctypes.data)


def host_check_cases():
    """(case, policy, min_valid, form, table): both widths, every form, the ladder and the loop, padded rows and CSR."""
    out = []
    for T, levels, scalar_lev in ((np.float32, (5, 9), 5), (np.float64, (3, 5), 2)):
        for i, k in enumerate((1, 2, 4, 5, 8, 17)):
            case = rs.make_case(T, k, levels[i % 2], n_tgt=67)
            for j, (policy, min_valid) in enumerate(((rs.ALL, 0.0), (rs.HEAVIEST, 0.0), (rs.ALL, 0.5), (rs.HEAVIEST, 1.0))):
                out.append((case, policy, min_valid, ("tight", "loose", "offset")[(i + j) % 3], "ell"))
        odd = rs.make_case(T, 4, scalar_lev, n_tgt=67)
        out.append((odd, rs.HEAVIEST, 0.5, "odd-pitch", "ell"))
        padded = rs.make_case(T, 6, levels[0], n_tgt=67, padded=True)
        ragged = rs.make_case(T, 0, levels[1], n_tgt=67, lengths=[0, 70, 1] + [3, 0, 5, 2] * 16)
        for policy, min_valid in ((rs.ALL, 0.5), (rs.HEAVIEST, 0.0), (rs.ALL, 1.0)):
            out.append((padded, policy, min_valid, "tight", "ell"))
            out.append((ragged, policy, min_valid, "loose", "csr"))
        out.append((ragged, rs.HEAVIEST, 0.5, "offset", "csr"))
    return out


def test_the_stand_in_passes_the_checks():
    kern = stand_in()
    for case, policy, min_valid, form, table in host_check_cases():
        check_case(kern, case, policy, min_valid, form, table)


@pytest.mark.parametrize("defect", DEFECTS)
def test_the_checks_catch_a_planted_defect(defect):
    kern = stand_in(defect)
    caught = 0
    for case, policy, min_valid, form, table in host_check_cases():
        try:
            check_case(kern, case, policy, min_valid, form, table)
        except AssertionError:
            caught += 1
    assert caught > 0, f"no check notices {defect}"


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_agree():
    """libatx_missing.so exports exactly the ATX_MISSING_API declarations of include/atx_missing.h, which native_missing binds; libatx
    itself is as it was."""
    import os

    import abi_checks

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "atx_missing.h")
    text = open(header).read()
    declared = abi_checks.header_declarations(header, "ATX_MISSING_API")
    assert declared == ["atx_missing_version", "atx_missing_last_error", "atx_regrid_ell_missing", "atx_regrid_csr_missing"]
    assert list(native_missing.SIGNATURES) == declared and not set(declared) & set(native.SIGNATURES)
    lib = native_missing.load()
    assert lib.atx_missing_version() == 420 and "#define ATX_MISSING_VERSION 420" in text
    if abi_checks.nm_tool():
        assert abi_checks.defined_dynamic_symbols(native_missing.lib_path())[0] == sorted(declared)


def test_no_kernel_uses_scratch_memory():
    """Read from the code objects inside libatx_missing.so (tools/kernel_resources.py; no GPU), as tests/test_host_api.py does for libatx."""
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.kernel_resources(native_missing.lib_path())
    kernels = [r for r in rows if "missing_kernel" in r["name"]]
    assert len(kernels) == 32  # 2 widths x (vector, scalar) x (7 fixed-k forms + CSR)
    assert [r["name"] for r in rows if r["scratch"] > 0 or r["lds"] > 0] == []


def test_abi_argument_validation_without_a_gpu():
    """Bad arguments are rejected before anything touches HIP, with the status codes of atx_regrid_ell / atx_regrid_csr."""
    lib = native_missing.load()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    ell, csr = lib.atx_regrid_ell_missing, lib.atx_regrid_csr_missing

    def ell_call(src=one, out=one, idx=one, w=one, n_src=8, n_tgt=8, k=4, n_lev=4, sp=4, op=4, dtype=0, layout=0, flags=0, policy=0, min_valid=0.0):
        return ell(src, out, idx, w, n_src, n_tgt, k, n_lev, sp, op, dtype, layout, flags, policy, min_valid, None)

    def csr_call(src=one, out=one, indptr=one, indices=one, data=one, n_src=8, n_tgt=8, nnz=8, n_lev=4, sp=4, op=4, dtype=0, layout=0, policy=0,
                 min_valid=0.0):
        return csr(src, out, indptr, indices, data, n_src, n_tgt, nnz, n_lev, sp, op, dtype, layout, policy, min_valid, None)

    assert ell_call(src=None) == native.EINVAL and b"null" in lib.atx_missing_last_error()
    assert ell_call(out=None) == native.EINVAL and ell_call(idx=None) == native.EINVAL
    assert ell_call(w=None) == native.EINVAL and b"null w" in lib.atx_missing_last_error()
    assert ell_call(k=0) == native.EINVAL and ell_call(k=65) == native.EINVAL
    assert ell_call(dtype=7) == native.EINVAL and ell_call(layout=5) == native.EINVAL and ell_call(flags=2) == native.EINVAL
    assert ell_call(sp=3) == native.ESHAPE and ell_call(op=3) == native.ESHAPE
    assert ell_call(policy=2) == native.EINVAL and b"policy" in lib.atx_missing_last_error()
    assert ell_call(policy=-1) == native.EINVAL
    for bad in (-0.1, 1.5, float("nan")):
        assert ell_call(min_valid=bad) == native.EINVAL and b"min_valid" in lib.atx_missing_last_error()
        assert csr_call(min_valid=bad) == native.EINVAL and b"min_valid" in lib.atx_missing_last_error()
    assert ell_call(layout=1, sp=8, op=8) == native.ENOTIMPL and b"column stacks" in lib.atx_missing_last_error()
    assert csr_call(layout=1, sp=8, op=8) == native.ENOTIMPL
    assert ell_call(out=None, idx=None, n_tgt=0) == native.OK  # no targets: validated, nothing launched
    assert ell_call(out=None, idx=None, n_tgt=0, policy=9) == native.EINVAL  # ... validated all the same
    assert csr_call(src=None) == native.EINVAL and csr_call(out=None) == native.EINVAL and csr_call(indptr=None) == native.EINVAL
    assert csr_call(indices=None) == native.EINVAL and csr_call(data=None) == native.EINVAL
    assert csr_call(indices=None, data=None, nnz=0, out=None, indptr=None, n_tgt=0) == native.OK
    assert csr_call(policy=2) == native.EINVAL and csr_call(sp=3) == native.ESHAPE and csr_call(nnz=-1) == native.ENOTIMPL
    with pytest.raises(RuntimeError, match="HBM-resident"):
        import torch

        native_missing.regrid_ell_missing(torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4, dtype=torch.int32), torch.zeros(4), n_src=4, n_tgt=4, k=1,
                                  n_lev=4, src_pitch=4, out_pitch=4, layout=native.COLUMNS, policy="all")
    with pytest.raises(ValueError, match="policy"):
        native_missing.missing_policy_code("some")
    assert native_missing.missing_policy_code("all") == native_missing.MISSING_ALL == 0 and native_missing.missing_policy_code("heaviest") == native_missing.MISSING_HEAVIEST == 1


# ---- the Python layers -------------------------------------------------------------------------------------------------------------
def tiny_matrix():
    lat, lon = np.array([10.0, 0.0, -10.0]), np.array([0.0, 10.0, 20.0])
    return dict(matrix_shape=np.array([3, 5]), matrix_data=np.array([0.5, 0.5, 0.25, 0.75, 1.0]), matrix_indices=np.array([0, 1, 1, 2, 4], dtype=np.int32),
                matrix_indptr=np.array([0, 2, 4, 5], dtype=np.int32), out_latitudes=lat, out_longitudes=lon)


def test_gather_plan_validates_the_policy():
    plan = GatherPlan(5, 3, index=np.array([[0, 1], [1, 2], [3, 4]]), weights=np.full((3, 2), 0.5))
    assert plan.apply_many([], missing="all", min_valid=0.5) == [] and plan.apply_many([], missing=None) == []
    with pytest.raises(ValueError, match="missing="):
        plan.apply_many([], missing="missing-if-all-missing")  # the filter's spellings are the filter's
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_valid"):
            plan.apply_many([], missing="heaviest", min_valid=bad)
    with pytest.raises(ValueError, match="program"):
        plan._missing_route("all", 0.0, prog=object())
    with pytest.raises(ValueError, match="mask"):
        plan._missing_route("all", 0.0, tgt_mask=object())
    assert plan._missing_route("all", 0.0) and plan._missing_route("heaviest", 1.0) and not plan._missing_route(None, 0.0)
    copy = GatherPlan(5, 3, index=np.array([0, 2, 4]))  # unweighted k = 1: a copy has nothing to renormalise
    assert not copy._missing_route("all", 0.0) and not copy._missing_route("heaviest", 0.5)


def test_filter_construction(caplog):
    from anemoi_transform_amd.core import reset_notes

    for spelling, policy in (("missing-if-all-missing", "all"), ("missing-if-heaviest-missing", "heaviest"), ("missing-if-any-missing", None), (None, None)):
        f = create_filter_by_name("regrid", matrix=tiny_matrix(), missing=spelling, min_valid=0.25)
        assert f.missing == policy and f.min_valid == 0.25
        # a regrid with a renormalising policy runs alone: the fused launch has no such kernel
        assert (fusion._gather_head(f) is None) == (policy is not None)
    assert create_filter_by_name("regrid", matrix=tiny_matrix()).missing is None
    assert create_filter_by_name("regrid", mask=np.array([0, 2]), missing="missing-if-all-missing").missing == "all"
    for bad in ("all", "missing-if-most-missing", "", 1):
        with pytest.raises(ValueError, match="missing"):
            create_filter_by_name("regrid", matrix=tiny_matrix(), missing=bad)
    for bad in (-0.1, 1.5, float("nan"), "0.5", None):
        with pytest.raises(ValueError, match="min_valid"):
            create_filter_by_name("regrid", matrix=tiny_matrix(), missing="missing-if-all-missing", min_valid=bad)

    def notes(fresh, **config):
        if fresh:
            reset_notes()
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger="anemoi_transform_amd"):
            create_filter_by_name("regrid", matrix=tiny_matrix(), **config)
        return [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING and "unpinned" in r.getMessage()]

    said = notes(True, missing="missing-if-all-missing")
    assert len(said) == 1 and "MIR" in said[0] and "in-tree" in said[0]
    assert notes(False, missing="missing-if-heaviest-missing") == []  # once per process ...
    assert any("unpinned" in r.getMessage() and r.levelno == logging.DEBUG for r in caplog.records)  # ... and still there for who asks
    assert notes(True, missing="missing-if-any-missing") == [] and notes(True) == []  # the plain route has nothing to say
