"""The checks of tests/gather_route_checks.py, run on the CPU against a numpy stand-in of ``native.regrid_ell`` / ``regrid_ell_batch`` /
``regrid_csr`` / ``last_gather_route`` that decides as the dispatcher of the gather does (the same conditions in the same order) and
walks the pitched buffers as the kernels do — workgroups dealt to the XCDs, (target, vector) items, the lanes of a vector, padded
rows, the head and the tail of a CSR row — once as it is (every case passes and lands on the route it declares) and once per planted
defect (the assertion that is there for it fails).  No deliberately broken kernel ever runs on a device.  A split program is finished
by the per-point stand-in of tests/test_pointwise_route_checks_catch_defects.py."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import gather_route_checks as G
import pointwise_route_checks as PWC
import test_pointwise_route_checks_catch_defects as PW
from anemoi_transform_amd import native

CPU = torch.device("cpu")


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


class StandIn:
    """What mirrors what — a change to a condition there is a change here:

    =====================================  =============================================================================
    here                                   csrc
    =====================================  =============================================================================
    ``regrid_ell_batch``, ``regrid_csr``   atx_regrid.hip ``regrid_ell_common``, ``regrid_csr_common`` (the split fallback)
    ``G.decide_cols_ell``                  atx_regrid_columns.inc ``regrid_cols_ell``, ``dispatch_cols_ell``, ``launch_cols_ell`` (uniform, runs, table in
                                           that order; the tile, its 48 KB clamp, the 64 KB limit)
    ``G.decide_cols_csr``                  ``regrid_cols_csr``, ``launch_cols_csr``
    ``G.decide_fields_ell`` / ``_csr``     atx_regrid_fields.inc ``dispatch_fields_ell``, ``regrid_fields_csr``
    ``_cols_ell``, ``_cols_csr``           the grids of the column kernels: workgroups to items
    ``_fields_ell``, ``_fields_csr``       the grids of the field-major kernels: lane = target
    ``_xcd_tile``, ``_xcd_stripe``         atx_common.hpp ``xcd_tile``, ``xcd_stripe``
    ``_items``, ``_ell_sum``, ``_csr_sum`` the kernels: one (target, vector) item, the sum from 0 in storage order, absent entries skipped
    ``_epilogue``                          the direct kernel's three epilogues, ``apply_level_tables``, ``apply_level_op``
    ``G.pick_tile``, ``G.tables_bytes``    atx_regrid_decl.hpp ``pick_tile``, atx_common.hpp ``level_tables_lds_bytes``
    ``G.uniform_form``, ``G.runs_form``    atx_common.hpp ``uniform_level_program``, ``runs_level_program``
    ``pw._apply``                          atx_common.hpp ``apply_level_op``
    =====================================  ============================================================================="""

    def __init__(self, k: G.Constants = G.K, defect: str | None = None):
        self.k, self.defect, self.route, self.tile = k, defect, None, 0
        self.pw = PW.StandIn(PWC.K)  # one operator on an array, and the per-point pass after a split

    def kernels(self) -> G.Kernels:
        return G.Kernels(regrid_ell=self.regrid_ell, regrid_ell_batch=self.regrid_ell_batch, regrid_csr=self.regrid_csr, last_gather_route=self.last_gather_route,
                         last_route=lambda: self.pw.route, level_program=self.pw.level_program, set_tuning=self.set_tuning)

    def set_tuning(self, tile: int) -> None:
        self.tile = tile

    def last_gather_route(self) -> str:
        if self.route is None:
            return "none"
        name = self.route.name()
        if self.defect == "a route mis-named":
            name = name.replace("/table/", "/uniform/")
        return name

    # ---- how workgroups are dealt to the XCDs ------------------------------------------------------------------------------------------
    def _xcd_tile(self, n: int) -> np.ndarray:
        b, X = np.arange(n), self.k.xcds
        x, r, per, rem = b % X, b // X, n // X, n % X
        return x * per + np.minimum(x, rem) + r

    def _xcd_stripe(self, n: int, g: int) -> np.ndarray:
        b, X = np.arange(n), self.k.xcds
        group = X * g
        n_full = n // group * group
        x, r = b % X, b // X
        dealt = np.where(b >= n_full, b, (r // g) * group + x * g + (r % g))
        if self.defect == "a stripe permutation visits one workgroup twice and another never" and n_full:
            dealt[1] = dealt[0]
        return dealt

    # ---- a program as the launchers see it ---------------------------------------------------------------------------------------------
    @staticmethod
    def _program(prog, n_stage, n_lev, dtype):
        if prog is None:
            return None, False, None
        P = prog.numpy().view(native.LEVEL_OP_DTYPE).reshape(-1, n_lev)[:n_stage]
        vec = getattr(prog, "vec_prog", {}).get(dtype)
        return P, getattr(prog, "host_prog", None) is not None, None if vec is None else vec.data_ptr()

    def _masked(self, mask, row, t):
        if mask is None:
            return None
        byte = mask[t if self.defect == "the mask indexed by table row in an ordered launch" else row]
        return byte == 1 if self.defect == "the mask byte tested as == 1" else byte != 0

    def _epilogue(self, T, acc, P, launch, c, C, ll, masked):
        """All stages on the elements of level ``ll`` in vector column ``c``."""
        if P is None:
            return acc
        kind, info = launch.epilogue, launch.form
        for s in range(P.shape[0]):
            if kind == "uniform":
                split, first, second = info[s]
                late = 1 if (self.defect == "the second piece of a uniform stage applied one vector late" and split < C) else 0
                e = first if c < split + late else second
            elif kind == "runs":
                off = 1 if self.defect == "a run boundary one level off" else 0
                e = [op for r, (start, op) in enumerate(info[s]) if ll >= start + (off if r else 0)][-1]
            elif kind == "table" and self.defect == "the table route reads the next stage's code byte":
                other = P[min(s + 1, P.shape[0] - 1), ll]
                e = np.zeros((), dtype=native.LEVEL_OP_DTYPE)
                e["op"], e["use_mask"], e["p0"], e["p1"] = other["op"], other["use_mask"], P[s, ll]["p0"], P[s, ll]["p1"]
            else:
                e = P[s, ll]
            acc = self.pw._apply(T, e, acc, masked, False)
        return acc

    # ---- the sums: from 0, in storage order, one rounding per product and per addition ---------------------------------------------------
    def _ell_sum(self, T, src, addr, I, W, pad):
        """``I`` / ``W`` [n, k]: the rows of the items; ``addr(p)``: where source point p's element is."""
        if W is None:
            return src[addr(I[:, 0].astype(np.int64))]
        acc = np.zeros(I.shape[0], dtype=T)
        spare = np.where(I[:, 0] >= 0, I[:, 0], 0)  # what an absent entry loads: the row's first column
        with np.errstate(all="ignore"):
            for j in range(I.shape[1]):
                present = I[:, j] >= 0 if pad else np.ones(I.shape[0], dtype=bool)
                term = W[:, j] * src[addr(np.where(present, I[:, j], spare).astype(np.int64))]
                new = term if (j == 0 and self.defect == "the sum started from the first product") else acc + term
                acc = np.where(present | (self.defect == "an absent padded entry added in"), new, acc)
        return acc

    def _csr_sum(self, T, src, addr, indptr, indices, data, sel, head=0):
        j0 = indptr[sel].astype(np.int64)
        n = indptr[sel + 1].astype(np.int64) - j0
        acc = np.zeros(sel.size, dtype=T)
        with np.errstate(all="ignore"):
            for j in range(int(n.max()) if sel.size else 0):
                has = j < n
                if head and j == head and self.defect == "the head kernel drops entry R":
                    continue
                at = np.where(has, j0 + j, 0)
                term = data[at] * src[addr(indices[at].astype(np.int64))]
                new = term if (j == 0 and self.defect == "the sum started from the first product") else acc + term
                acc = np.where(has, new, acc)
        return acc

    # ---- ATX_COLUMNS: (target, vector) items ------------------------------------------------------------------------------------------------
    def _items(self, T, batch, t, cc, launch, n_lev, sp, op, row_sum, P, mask, rows):
        """Every item (table row t, vector column cc) of every stack: the sum of each of its VEC elements, the epilogue, the store."""
        VEC = launch.vec
        C = ceil_div(n_lev, VEC)
        for src_t, out_t in batch:
            src, out = src_t.numpy(), out_t.numpy()
            late = []
            for c in range(C):
                sel = t[cc == c]
                row = sel if rows is None else rows[sel].astype(np.int64)
                masked = self._masked(mask, row, sel) if P is not None else None
                for e in range(VEC):
                    l = c * VEC + e  # (an element past the last level: padding inside the pitch, the last level's operators)
                    acc = row_sum(src, lambda p, l=l: p * sp + l, sel)
                    acc = self._epilogue(T, acc, P, launch, c, C, min(l, n_lev - 1), masked)
                    out[row * op + l] = acc
                    if l >= n_lev and self.defect == "the last partial vector's spare lanes stored past the pitch":
                        late.append((row * op + op + (l - n_lev), acc))
            for at, acc in late:
                out[at] = acc

    def _tiles(self, launch, n_tgt, n_lev):
        """The tiled kernels: tiles of targets dealt to the XCDs, every vector column of every target."""
        C = ceil_div(n_lev, launch.vec)
        n_tiles = ceil_div(n_tgt, launch.tile)
        dealt = self._xcd_stripe(n_tiles, launch.stripe) if launch.stripe else self._xcd_tile(n_tiles)
        t = (dealt[:, None] * launch.tile + np.arange(launch.tile)[None, :]).reshape(-1)
        t = t[t < n_tgt]
        return np.repeat(t, C), np.tile(np.arange(C), t.size)

    def _cols_ell(self, T, batch, idx, w, n_tgt, k, n_lev, sp, op, pad, P, host, vec_ptr, mask, rows) -> bool:
        """True: the program does not fit beside the tile (ATX_SPLIT_PROGRAM)."""
        launch = G.decide_cols_ell(T, [x.data_ptr() for pair in batch for x in pair], n_tgt, k, n_lev, sp, op, pad, w is not None, P, host, vec_ptr, mask is not None,
                                   rows is not None, self.tile, self.k)
        if launch is None:
            return True
        self.route = launch
        if launch.kernel == "direct":  # one (target, vector) item per lane, kEllBlock of them per workgroup
            C, block = ceil_div(n_lev, launch.vec), self.k.ell_block
            n_items = n_tgt * C
            n_blocks = ceil_div(n_items, block)
            dealt = self._xcd_stripe(n_blocks, launch.stripe) if launch.stripe else self._xcd_tile(n_blocks)
            q = (dealt[:, None] * block + np.arange(block)[None, :]).reshape(-1)
            q = q[q < n_items]
            t, cc = q // C, q % C
        else:
            t, cc = self._tiles(launch, n_tgt, n_lev)
        self._items(T, batch, t, cc, launch, n_lev, sp, op, lambda src, addr, sel: self._ell_sum(T, src, addr, idx[sel], None if w is None else w[sel], pad), P, mask, rows)
        return False

    def _cols_csr(self, T, src_t, out_t, indptr, indices, data, n_tgt, nnz, n_lev, sp, op, P, mask, rows) -> bool:
        launch = G.decide_cols_csr(T, [src_t.data_ptr(), out_t.data_ptr()], n_tgt, nnz, n_lev, sp, op, P, rows is not None, self.tile, self.k)
        if launch is None:
            return True
        self.route = launch
        t, cc = self._tiles(launch, n_tgt, n_lev)
        self._items(T, [(src_t, out_t)], t, cc, launch, n_lev, sp, op, lambda src, addr, sel: self._csr_sum(T, src, addr, indptr, indices, data, sel), P, mask, rows)
        return False

    # ---- ATX_FIELDS: lane = target ------------------------------------------------------------------------------------------------------------
    def _lanes(self, T, src_t, out_t, launch, n_tgt, n_lev, sp, op, row_sum, P, mask, skip=None):
        self.route = launch
        src, out = src_t.numpy(), out_t.numpy()
        n_tiles = ceil_div(n_tgt, self.k.block)
        t = (self._xcd_tile(n_tiles)[:, None] * self.k.block + np.arange(self.k.block)[None, :]).reshape(-1)
        t = t[t < n_tgt]
        masked = self._masked(mask, t, t) if P is not None else None
        for l in range(n_lev):
            if skip is not None and skip(l):
                continue
            acc = row_sum(src, lambda p, l=l: l * sp + p, t)
            out[l * op + t] = self._epilogue(T, acc, P, launch, 0, 1, l, masked)

    def _fields_ell(self, T, src_t, out_t, idx, w, n_tgt, k, n_lev, sp, op, pad, P, mask):
        self._lanes(T, src_t, out_t, G.decide_fields_ell(k, pad, w is not None, P), n_tgt, n_lev, sp, op,
                    lambda src, addr, sel: self._ell_sum(T, src, addr, idx[sel], None if w is None else w[sel], pad), P, mask)

    def _fields_csr(self, T, src_t, out_t, indptr, indices, data, n_tgt, nnz, n_lev, sp, op, P, mask):
        launch, chunk = G.decide_fields_csr(n_tgt, nnz, P, self.k), self.k.fields_chunk
        skip = (lambda l: l % chunk == chunk - 1) if (launch.kernel == "long" and self.defect == "the 16-field chunk's last field skipped") else None
        self._lanes(T, src_t, out_t, launch, n_tgt, n_lev, sp, op, lambda src, addr, sel: self._csr_sum(T, src, addr, indptr, indices, data, sel, head=launch.head), P, mask, skip)

    # ---- the entry points -------------------------------------------------------------------------------------------------------------------------
    def _finish(self, out_t, prog, n_stage, n_tgt, n_lev, op, layout, tgt_mask, rows):
        """The split fallback's second half: the program on the gather's output, in place, the mask indexed by output row."""
        if tgt_mask is not None and rows is not None and self.defect == "the split fallback applies the program to the table-order row":
            moved = tgt_mask.numpy().copy()
            moved[rows] = tgt_mask.numpy()[:n_tgt]
            tgt_mask = torch.from_numpy(moved)
        self.pw.pointwise_stack(out_t, out_t, n_pts=n_tgt, n_lev=n_lev, x_pitch=op, y_pitch=op, layout=layout, prog=prog, n_stage=n_stage, point_mask=tgt_mask)

    def regrid_ell(self, src, out, idx, w, **kw):
        self.regrid_ell_batch([src], [out], idx, w, **kw)

    def regrid_ell_batch(self, srcs, outs, idx, w, *, n_src, n_tgt, k, n_lev, src_pitch, out_pitch, layout, prog=None, n_stage=0, tgt_mask=None, padded=False, tgt_rows=None):
        self.route = None
        assert 1 <= k <= 64 and (w is not None or k == 1) and (not padded or w is not None) and (tgt_rows is None or layout == native.COLUMNS)
        if n_tgt == 0:
            return
        T = np.float32 if srcs[0].dtype == torch.float32 else np.float64
        idx, w = idx.numpy().reshape(n_tgt, k), None if w is None else w.numpy().reshape(n_tgt, k)
        mask, rows = None if tgt_mask is None else tgt_mask.numpy(), None if tgt_rows is None else tgt_rows.numpy()
        P, host, vec_ptr = self._program(prog, n_stage, n_lev, srcs[0].dtype)
        for first in range(0, len(srcs), self.k.max_batch):
            batch = list(zip(srcs[first: first + self.k.max_batch], outs[first: first + self.k.max_batch]))

            def run(P, host, vec_ptr, mask):
                if layout == native.COLUMNS:
                    return self._cols_ell(T, batch, idx, w, n_tgt, k, n_lev, src_pitch, out_pitch, padded, P, host, vec_ptr, mask, rows)
                for src_t, out_t in batch:
                    self._fields_ell(T, src_t, out_t, idx, w, n_tgt, k, n_lev, src_pitch, out_pitch, padded, P, mask)
                return False

            if run(P, host, vec_ptr, mask):
                assert not run(None, False, None, None)
                self.route.epilogue = "split"
                for _, out_t in batch:
                    self._finish(out_t, prog, n_stage, n_tgt, n_lev, out_pitch, layout, tgt_mask, rows)

    def regrid_csr(self, src, out, indptr, indices, data, *, n_src, n_tgt, nnz, n_lev, src_pitch, out_pitch, layout, prog=None, n_stage=0, tgt_mask=None, tgt_rows=None):
        self.route = None
        if n_tgt == 0:
            return
        T = np.float32 if src.dtype == torch.float32 else np.float64
        indptr, indices, data = indptr.numpy(), indices.numpy(), data.numpy()
        mask, rows = None if tgt_mask is None else tgt_mask.numpy(), None if tgt_rows is None else tgt_rows.numpy()
        P, _, _ = self._program(prog, n_stage, n_lev, src.dtype)

        def run(P, mask):
            if layout == native.COLUMNS:
                return self._cols_csr(T, src, out, indptr, indices, data, n_tgt, nnz, n_lev, src_pitch, out_pitch, P, mask, rows)
            assert rows is None
            self._fields_csr(T, src, out, indptr, indices, data, n_tgt, nnz, n_lev, src_pitch, out_pitch, P, mask)
            return False

        if run(P, mask):
            assert not run(None, None)
            self.route.epilogue = "split"
            self._finish(out, prog.detach().clone(), n_stage, n_tgt, n_lev, out_pitch, layout, tgt_mask, rows)  # (the CSR entry point has no companions to hand on)


# ---- the runs -----------------------------------------------------------------------------------------------------------------------
CASES = {c.name: c for c in G.all_cases()}


def run(kern, *parts):
    """Every case whose name holds one of ``parts``."""
    chosen = [c for name, c in CASES.items() if any(p in name for p in parts)]
    assert chosen, parts
    groups = {}
    for case in chosen:
        G.check_case(kern, CPU, case, groups)


def test_the_stand_in_passes_every_case_on_its_route():
    kern = StandIn().kernels()
    groups, taken = {}, set()
    for case in CASES.values():
        taken.add(G.route_class(G.check_case(kern, CPU, case, groups)))
    assert taken == set(G.ROUTE_CLASSES)
    G.check_nothing_launched(kern, CPU)


def test_the_cases_name_every_route_and_stay_small():
    cases = list(CASES.values())
    assert G.declared_route_classes(cases) == set(G.ROUTE_CLASSES)
    names = {c.route for c in cases}
    for k in (1, 3, 4, 5, 8, 12, 16):  # the compile-time k the direct epilogues are run at
        for epilogue in ("uniform", "runs", "table"):
            assert any(f"cols_ell/direct/{epilogue}/vec/k{k}/" in n for n in names), (k, epilogue)
    for word in ("padded", "pure", "stripe", "ordered"):
        assert any(f"/{word}" in n for n in names), word
    assert max(c.n_tgt * c.n_lev * c.n_stack for c in cases) <= 140_000 and sum(c.n_tgt * c.n_lev * c.n_stack for c in cases) <= 4_000_000


def test_the_native_double_names_the_route_of_every_case():
    """tests/native_double.py decides as the dispatcher does (the same ``G.decide_*``): on the buffers of every case it names the case's route,
    and its scipy / numpy statements give the case's expectation."""
    import native_double

    def stack(case, n_pts, pitch, offset, values=None):
        rows, row_len = (n_pts, case.n_lev) if case.layout == G.COLUMNS else (case.n_lev, n_pts)
        room = torch.zeros(rows * pitch + offset + 16, dtype=torch.float32 if case.np_dtype == np.float32 else torch.float64)
        assert room.data_ptr() % 16 == 0
        t = room[offset: offset + rows * pitch].view(rows, pitch)
        if values is not None:
            t[:, :row_len] = torch.from_numpy(np.array(values.T if case.layout == G.COLUMNS else values))
        return t

    try:
        for case in CASES.values():
            if case.n_tgt > 5000:
                continue
            native_double.np.seterr(all="ignore")
            p = G.problem(case)
            srcs = [stack(case, case.n_src, case.sp(), 0, x) for x in p.xs]
            outs = [stack(case, case.n_tgt, case.op(), case.offset) for _ in p.xs]
            visit = p.order if case.ordered else np.arange(case.n_tgt)
            prog = G.build_program(StandIn().kernels(), case, CPU)
            kw = dict(n_src=case.n_src, n_tgt=case.n_tgt, n_lev=case.n_lev, src_pitch=case.sp(), out_pitch=case.op(), layout=case.layout, prog=prog,
                      n_stage=0 if case.stages is None else len(case.stages), tgt_mask=None if p.mask is None else torch.from_numpy(p.mask.copy()),
                      tgt_rows=torch.from_numpy(p.order.copy()) if case.ordered else None)
            native_double.set_tuning(case.tile)
            if case.table == "ell":
                idx, w = torch.from_numpy(np.ascontiguousarray(p.idx[visit])), (torch.from_numpy(np.ascontiguousarray(p.w[visit])) if case.weighted else None)
                native_double.regrid_ell_batch(srcs, outs, idx, w, k=case.k, padded=case.padded, **kw)
            else:
                lengths = np.diff(p.indptr)[visit]
                take = np.concatenate([np.arange(p.indptr[r], p.indptr[r + 1]) for r in visit]).astype(np.int64)
                indptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32))
                native_double.regrid_csr(srcs[0], outs[0], indptr, torch.from_numpy(p.indices[take].copy()), torch.from_numpy(p.data[take].copy()), nnz=int(p.indptr[-1]), **kw)
            assert native_double.last_gather_route() == case.route, case.name
            for out, want in zip(outs, p.want):
                got = native_double._levels(out, case.n_tgt, case.n_lev, case.layout)
                assert np.array_equal(got, want, equal_nan=True), case.name
    finally:
        native_double.set_tuning(0)


# defect -> (cases that meet it, the assertion that catches it)
DEFECTS = {
    "the second piece of a uniform stage applied one vector late": (("direct-uniform-two-pieces-f32-k4",), r"values differ from numpy's bits|NaN where numpy has none"),
    "a run boundary one level off": (("direct-runs-4-runs-f64-k4",), r"values differ from numpy's bits|NaN where numpy has none"),
    "the table route reads the next stage's code byte": (("direct-table-mask-on-some-levels-f32-k4",), r"values differ from numpy's bits|NaN where numpy has none"),
    "the mask indexed by table row in an ordered launch": (("direct-uniform-f64-k5-ordered",), r"NaN where numpy has none, or none where numpy has one"),
    "the mask byte tested as == 1": (("tiled-general-f32-k9-padded-ordered",), r"NaN where numpy has none, or none where numpy has one"),
    "an absent padded entry added in": (("direct-runs-f32-k3-padded",), r"values differ from numpy's bits|NaN where numpy has none"),
    "the sum started from the first product": (("shape-plain-f32-k1-weighted",), r"values differ from numpy's bits"),
    "the last partial vector's spare lanes stored past the pitch": (("shape-uniform-f32-L5-",), r"values differ from numpy's bits|NaN where numpy has none|canary written"),
    "the split fallback applies the program to the table-order row": (("split-ell-f64-k4-ordered-L",), r"NaN where numpy has none, or none where numpy has one"),
    "the head kernel drops entry R": (("fields-csr-head4-f32-L1-",), r"values differ from numpy's bits|NaN where numpy has none"),
    "the 16-field chunk's last field skipped": (("fields-csr-long-f64-L17-",), r"level 15 point \d+: kernel np\.float64\(12345\.0\)"),
    "a stripe permutation visits one workgroup twice and another never": (("shape-plain-f32-stripes-past-one-group",), r"kernel np\.float32\(12345\.0\)"),
    "a route mis-named": (("direct-table-f32-k4",), r"route cols_ell/direct/uniform/vec/k4/\S+, the case is written for cols_ell/direct/table/vec/k4/"),
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_check_catches_its_defect(defect):
    parts, message = DEFECTS[defect]
    with pytest.raises(AssertionError, match=message):
        run(StandIn(defect=defect).kernels(), *parts)


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_defect_is_caught_by_its_cases_alone(defect):
    """The cases named for a defect pass on the clean stand-in: what fails above is the defect."""
    run(StandIn().kernels(), *DEFECTS[defect][0])
