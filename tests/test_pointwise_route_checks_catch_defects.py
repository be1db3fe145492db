"""The checks of tests/pointwise_route_checks.py, run on the CPU against a numpy stand-in of ``native.pointwise_stack`` /
``native.last_route`` that decides as the dispatcher of csrc/atx_pointwise.hip does (the same conditions in the same order) and
walks the pitched buffers as the kernels do — vectors, slots, pieces, runs, the lanes and the tail of a field — once as it is
(every case passes and lands on the route it declares) and once per planted defect (the assertion that is there for it fails).  No
deliberately broken kernel ever runs on a device.  The stand-in's constants are small; the cases take them as an argument."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import pointwise_route_checks as C
from anemoi_transform_amd import native

CPU = torch.device("cpu")
SMALL = C.Constants(block=8, unroll=2, max_active=4, max_uniform=4, max_runs=4, max_stages=8, lds=4096, stream_grid=8)
NAN = float("nan")


def roundup16(n: int) -> int:
    return (n + 15) & ~15


class StandIn:
    """What mirrors what — a change to a condition there is a change here (line numbers as of this file's writing):

    =====================================  =============================================================================
    here                                   csrc
    =====================================  =============================================================================
    ``_apply``                             atx_common.hpp:438 ``apply_level_op`` (and its ``_vec`` / ``_params`` twins)
    ``_same``, ``_uniform``                atx_common.hpp:782 ``uniform_level_program``
    ``_runs``                              atx_common.hpp:833 ``runs_level_program``
    ``_mixed_vectors``                     atx_common.hpp:903 ``program_has_mixed_vectors``
    ``roundup16(...)`` (level tables)      atx_common.hpp:613 ``level_tables_lds_bytes``; 16 / 24 bytes: ``sizeof(LevelOp<T>)``
    ``_columns``: wide, slots, tight, Cp   atx_pointwise.hip:745 ``pointwise_columns``
    ``_columns``: the blocks "# route_*"   atx_pointwise.hip:567 ``route_sparse``, :592 ``route_uniform``, :621 ``route_runs``, :644
                                           ``route_table``, :659 ``route_typed``, :686 ``route_levels``, :707 ``route_flat``, :724
                                           ``route_row_chunk``, in the order of the ``routes[]`` table of ``pointwise_columns``
    ``_fields``                            atx_pointwise.hip:767 ``pointwise_fields``, :425 ``pointwise_fields_rows_kernel``
    ``pointwise_stack``, ``_run``          atx_pointwise.hip:806 ``atx_pointwise_stack`` (the split program)
    =====================================  ============================================================================="""

    def __init__(self, k: C.Constants = SMALL, defect: str | None = None):
        self.k, self.defect, self.route = k, defect, "none"

    def kernels(self) -> C.Kernels:
        return C.Kernels(pointwise_stack=self.pointwise_stack, last_route=lambda: self.route, level_program=self.level_program)

    def level_program(self, stages, device):
        prog = native.level_program(stages, device)  # (host_prog attached; the per-vector tables need the library and a device)
        prog.vec_prog = {tdt: torch.zeros(64, dtype=torch.uint8) for tdt in (torch.float32, torch.float64)}  # read for presence and alignment only
        return prog

    # ---- one operator on an array of elements: apply_level_op of csrc/atx_common.hpp -------------------------------------------------
    def _apply(self, T, e, v, masked, trans):
        op, use_mask = int(e["op"]), int(e["use_mask"]) != 0
        p0, p1 = T(e["p0"]), T(e["p1"])
        if self.defect == "parameter used in float64 and the result rounded":
            p0, p1 = np.float64(e["p0"]), np.float64(e["p1"])
        with np.errstate(all="ignore"):
            if op == native.OP_COPY:
                y = v.copy()
            elif op == native.OP_AFFINE:
                if trans and self.defect == "the TRANS twin contracts AFFINE into an fma":
                    y = (v.astype(np.longdouble) * p0 + p1).astype(T)
                else:
                    y = (v * p0 + p1).astype(T)
            elif op == native.OP_AFFINE_INV:
                y = ((v - p1) / p0).astype(T)
            elif op == native.OP_MUL:
                y = (v * p0).astype(T)
            elif op == native.OP_DIV:
                y = (v / p0).astype(T)
            elif op == native.OP_CLIP:
                y = v.copy()
                if not np.isnan(p0):
                    y = np.where(y < p0, T(p0), y)
                if not np.isnan(p1):
                    y = np.where(y > p1, T(p1), y)
            elif op == native.OP_IMPUTE_NAN:
                y = np.where(v != v, T(p0), v)
            elif op == native.OP_EXP:
                y = np.exp(v.astype(np.longdouble)).astype(T)
            elif op == native.OP_LOG:
                y = np.log(v.astype(np.longdouble)).astype(T)
            else:
                assert op == native.OP_SET_NAN
                y = np.full_like(v, NAN)
        if masked is not None and (use_mask or self.defect == "mask read although the stage does not use it"):
            y = np.where(masked, T(NAN), y)
        return y

    def _stage_order(self, n_stage):
        if self.defect == "stage order swapped":
            return list(reversed(range(n_stage)))
        if self.defect == "stages beyond the 4th ignored":
            return list(range(min(n_stage, 4)))
        return list(range(n_stage))

    def _masked(self, mask, n_pts):
        """The mask of each point, as a column beside its levels."""
        if mask is None:
            return None
        first = 1 if self.defect == "mask byte of point p + 1" else 0
        return (mask[first: first + n_pts] != 0)[:, None]

    # ---- what the dispatcher asks of a program ------------------------------------------------------------------------------------------
    def _same(self, T, a, b, rounded=True):
        if int(a["op"]) != int(b["op"]) or (int(a["use_mask"]) != 0) != (int(b["use_mask"]) != 0):
            return False
        if not rounded:
            return a["p0"].tobytes() == b["p0"].tobytes() and a["p1"].tobytes() == b["p1"].tobytes()
        return T(a["p0"]).tobytes() == T(b["p0"]).tobytes() and T(a["p1"]).tobytes() == T(b["p1"]).tobytes()

    @staticmethod
    def _active(e) -> bool:
        return int(e["op"]) != native.OP_COPY or int(e["use_mask"]) != 0

    def _uniform(self, T, P, have_mask, n_lev, vec):
        """uniform_level_program: per stage (split column, first piece, second piece), or None."""
        n_stage = P.shape[0]
        if n_stage > self.k.max_uniform:
            return None
        C_ = -(-n_lev // vec)
        out = []
        for s in range(n_stage):
            row = P[s]
            l = 1
            while l < n_lev and self._same(T, row[l], row[0]):
                l += 1
            if l == n_lev:
                out.append((C_, row[0], row[0]))
                continue
            if l % vec:
                return None
            if any(not self._same(T, row[j], row[l]) for j in range(l + 1, n_lev)):
                return None
            out.append((l // vec, row[0], row[l]))
        if any((int(a["use_mask"]) or int(b["use_mask"])) and not have_mask for _, a, b in out):
            return None
        return out

    def _runs(self, T, P, have_mask, n_lev):
        """runs_level_program: per stage [(first level, operator)], or None."""
        if P.shape[0] > self.k.max_uniform:
            return None
        rounded = self.defect != "runs merged on the float64 parameters"
        out = []
        for row in P:
            runs = []
            for l in range(n_lev):
                if runs and self._same(T, row[l], runs[-1][1], rounded):
                    continue
                if len(runs) == self.k.max_runs:
                    return None
                runs.append((l, row[l]))
            if any(int(e["use_mask"]) and not have_mask for _, e in runs):
                return None
            out.append(runs)
        return out

    def _mixed_vectors(self, T, P, n_lev, vec):
        return any(not self._same(T, row[l], row[l0]) for row in P for l0 in range(0, n_lev, vec) for l in range(l0 + 1, min(l0 + vec, n_lev)))

    # ---- ATX_COLUMNS ------------------------------------------------------------------------------------------------------------------------
    def _columns(self, T, xa, ya, x_ptr, y_ptr, n_pts, n_lev, xp, yp, P, host, vec_prog, mask):
        k, size = self.k, np.dtype(T).itemsize
        VEC = 16 // size
        n_stage = P.shape[0]
        in_place = x_ptr == y_ptr and xp == yp
        covered = -(-n_lev // VEC) * VEC
        wide = x_ptr % 16 == 0 and y_ptr % 16 == 0 and xp % VEC == 0 and yp % VEC == 0 and covered <= xp and covered <= yp
        C_ = covered // VEC if wide else n_lev
        slots = wide and yp == xp
        tight = xp == C_ * VEC
        Cp = xp // VEC if slots else 0
        have_vec = vec_prog is not None
        trans = (not host) or any(int(e["op"]) in (native.OP_EXP, native.OP_LOG) for e in P.reshape(-1))
        rx, ry = np.arange(n_pts) * xp, np.arange(n_pts) * yp
        masked = self._masked(mask, n_pts)

        def column_active(c, vec):
            return any(self._active(P[s, l]) for s in range(n_stage) for l in range(c * vec, min((c + 1) * vec, n_lev)))

        def levels_of(c, vec):  # the vector's elements and the level whose operator each takes (the padding repeats the last level's)
            return [(l, min(l, n_lev - 1)) for l in range(c * vec, (c + 1) * vec)]

        def by_level(c, vec, tr=trans):
            """All stages on vector column c, every level its own operator."""
            for l, ll in levels_of(c, vec):
                v = xa[rx + l]
                for s in self._stage_order(n_stage):
                    v = self._apply(T, P[s, ll], v, None if masked is None else masked[:, 0], tr)
                ya[ry + l] = v

        def idle(c, vec):
            """An untouched vector of an in-place call: nothing moves."""
            if self.defect == "idle piece rewritten in place through x * 1 + 0":
                with np.errstate(all="ignore"):
                    for l, _ in levels_of(c, vec):
                        ya[ry + l] = xa[rx + l] * T(1) + T(0)

        # route_sparse
        if in_place and wide and host and have_vec:
            limit = k.max_active + (1 if self.defect == "17th sparse column aliased to the first" else 0)
            cols = [c for c in range(C_) if column_active(c, VEC)]
            if len(cols) <= limit:
                if not cols:
                    return "none"
                if 3 * len(cols) <= C_:
                    for a in range(len(cols)):
                        by_level(cols[a] if a < k.max_active else cols[0], VEC, tr=True)
                    return "sparse"
        # route_uniform
        uni = self._uniform(T, P, mask is not None, n_lev, VEC) if (slots and host) else None
        if uni is not None:
            late = 1 if self.defect == "two-piece split one vector late" else 0
            for c in range(Cp):
                if c >= C_:
                    if self.defect == "a padding slot of a loose pitch written":
                        for e in range(VEC):
                            ya[ry + c * VEC + e] = xa[rx + c * VEC + e]
                    continue
                chosen = [(a if c < split + (late if split < C_ else 0) else b) for split, a, b in uni]
                if in_place and not any(self._active(e) for e in chosen):
                    idle(c, VEC)
                    continue
                for l, _ in levels_of(c, VEC):
                    v = xa[rx + l]
                    for s in self._stage_order(n_stage):
                        v = self._apply(T, chosen[s], v, None if masked is None else masked[:, 0], trans)
                    ya[ry + l] = v
            return "uniform"
        # route_runs
        runs = self._runs(T, P, mask is not None, n_lev) if (slots and host and size == 4 and n_stage >= 2) else None
        if runs is not None:
            off = 1 if self.defect == "a run boundary one level off" else 0
            for c in range(min(Cp, C_)):
                for l, _ in levels_of(c, VEC):
                    v = xa[rx + l]
                    for s in self._stage_order(n_stage):
                        e = [op for r, (first, op) in enumerate(runs[s]) if l >= first + (off if r else 0)][-1]
                        v = self._apply(T, e, v, None if masked is None else masked[:, 0], trans)
                    ya[ry + l] = v
            return "runs"

        def sweep(vec, cols):
            for c in range(cols):
                if in_place and not column_active(c, vec):
                    idle(c, vec)
                    continue
                by_level(c, vec)
            if self.defect == "the padding of a partial last vector written beyond the vector" and vec > 1 and cols * vec < yp:
                ya[ry + cols * vec] = xa[rx + min(cols * vec, xp - 1)]

        # route_table
        if slots and tight and have_vec and mask is None and size == 4 and n_stage == 1 and not (host and self._mixed_vectors(T, P, n_lev, VEC)):
            sweep(VEC, C_)
            return "table"
        # route_typed
        if slots and tight and n_stage == 1 and (size == 8 or in_place) and have_vec and vec_prog % 16 == 0 and host:
            one_kind = all(int(P[0, l]["op"]) == int(P[0, l0]["op"]) and (int(P[0, l]["use_mask"]) != 0) == (int(P[0, l0]["use_mask"]) != 0)
                           for l0 in range(0, n_lev, VEC) for l in range(l0, min(l0 + VEC, n_lev)))
            uses_mask = any(int(e["use_mask"]) for e in P[0])
            if one_kind and (size == 8 or not (uses_mask and mask is not None)):
                sweep(VEC, C_)
                return "typed"
        # route_levels, route_flat
        if slots and tight:
            if roundup16(n_stage * C_ * VEC * (2 * size + 1)) + C_ <= k.lds:
                sweep(VEC, C_)
                return "levels"
            lds_flat = n_stage * C_ * (16 if size == 4 else 24) + C_
            if lds_flat > k.lds and n_stage > 1:
                return "split"
            assert lds_flat <= k.lds
            sweep(VEC, C_)
            return "flat"
        # route_row_chunk
        vec = VEC if wide else 1
        lds_rows = roundup16(n_stage * C_ * vec * (2 * size + 1))
        if lds_rows > k.lds and n_stage > 1:
            return "split"
        assert lds_rows <= k.lds
        sweep(vec, C_)
        return "row_chunk" if wide else "row_chunk_scalar"

    # ---- ATX_FIELDS: pointwise_fields_rows_kernel -----------------------------------------------------------------------------------------
    def _fields(self, T, xa, ya, x_ptr, y_ptr, n_pts, n_lev, xp, yp, P, host, mask):
        k, size = self.k, np.dtype(T).itemsize
        VEC = 16 // size
        n_stage = P.shape[0]
        in_place = x_ptr == y_ptr and xp == yp
        vec_ok = x_ptr % 16 == 0 and y_ptr % 16 == 0 and xp % VEC == 0 and yp % VEC == 0
        vec = VEC if vec_ok else 1
        U = 1 if size == 4 else 2  # vectors per lane, kBlock apart
        trans = (not host) or any(int(e["op"]) in (native.OP_EXP, native.OP_LOG) for e in P.reshape(-1))
        n_vec = n_pts // vec
        vi = np.arange(n_vec)
        if self.defect == "the float64 fields lane's second vector dropped" and U == 2:
            vi = vi[(vi % (k.block * U)) < k.block]
        body = (vi[:, None] * vec + np.arange(vec)[None, :]).reshape(-1)
        tail = np.arange(n_vec * vec, n_pts)
        tail_mask_at = tail
        if self.defect == "tail points dropped":
            tail = tail_mask_at = tail[:0]
        elif self.defect == "tail points masked by vector index":
            tail_mask_at = n_vec + np.arange(tail.size)
        pts, mask_at = np.concatenate([body, tail]), np.concatenate([body, tail_mask_at])
        masked = None if mask is None else mask[mask_at] != 0
        for l in range(n_lev):
            if not any(self._active(P[s, l]) for s in range(n_stage)) and in_place:
                continue
            v = xa[l * xp + pts]
            for s in self._stage_order(n_stage):
                v = self._apply(T, P[s, l], v, masked, trans)
            ya[l * yp + pts] = v
        return "fields" if vec_ok else "fields_scalar"

    # ---- atx_pointwise_stack ------------------------------------------------------------------------------------------------------------------
    def pointwise_stack(self, x, y, *, n_pts, n_lev, x_pitch, y_pitch, layout, prog, n_stage, point_mask=None):
        self.route = "none"
        if n_pts == 0:
            return
        T = np.float32 if x.dtype == torch.float32 else np.float64
        P = prog.numpy().view(native.LEVEL_OP_DTYPE).reshape(-1, n_lev)[:n_stage]
        host = getattr(prog, "host_prog", None) is not None
        vec = getattr(prog, "vec_prog", {}).get(x.dtype)
        mask = None if point_mask is None else point_mask.numpy()
        self._run(T, x.numpy(), y.numpy(), x.data_ptr(), y.data_ptr(), n_pts, n_lev, x_pitch, y_pitch, layout, P, host,
                  None if vec is None else vec.data_ptr(), mask)

    def _run(self, T, xa, ya, x_ptr, y_ptr, n_pts, n_lev, xp, yp, layout, P, host, vec_prog, mask):
        if layout == native.COLUMNS:
            route = self._columns(T, xa, ya, x_ptr, y_ptr, n_pts, n_lev, xp, yp, P, host, vec_prog, mask)
        else:
            route = self._fields(T, xa, ya, x_ptr, y_ptr, n_pts, n_lev, xp, yp, P, host, mask)
        if route != "split":
            self.route = route
            return
        first = P.shape[0] // 2  # the stages in two halves, the second in place; vec_prog does not travel with a part
        self._run(T, xa, ya, x_ptr, y_ptr, n_pts, n_lev, xp, yp, layout, P[:first], host, None, mask)
        self.route = "none"
        self._run(T, ya, ya, y_ptr, y_ptr, n_pts, n_lev, yp, yp, layout, P[first:], host, None, mask)


# ---- the runs -----------------------------------------------------------------------------------------------------------------------
CASES = {c.name: c for c in C.all_cases(SMALL)}


def run(kern, *parts):
    """Every case whose name holds one of ``parts``."""
    chosen = [c for name, c in CASES.items() if any(p in name for p in parts)]
    assert chosen, parts
    for case in chosen:
        C.check_case(kern, CPU, case)


def test_the_stand_in_passes_every_case_on_its_route():
    kern = StandIn().kernels()
    taken = set()
    for case in CASES.values():
        taken |= set(C.check_case(kern, CPU, case).values())
    assert taken - {"none"} == set(C.ROUTES)
    C.check_no_points(kern, CPU)


def test_the_cases_name_every_route_at_the_library_s_constants():
    cases = C.all_cases(C.K)
    assert C.declared_routes(cases) == set(C.ROUTES)
    assert max(c.n_pts * c.n_lev for c in cases) <= 40 * 2001 and max(c.n_pts for c in cases) <= 5000


# defect -> (cases that meet it, the assertion that catches it)
DEFECTS = {
    "two-piece split one vector late": (("uniform-two-pieces-f32-L25",), r"values differ from numpy's bits"),
    "a run boundary one level off": (("runs-3-f32",), r"values differ from numpy's bits"),
    "runs merged on the float64 parameters": (("runs-merge-after-rounding",), r"route levels, the case is written for runs"),
    "the padding of a partial last vector written beyond the vector": (("row-chunk-unequal-pitches-f32-L25",), r"padding written: row 0 element 28 "),
    "a padding slot of a loose pitch written": (("uniform-loose+1-f64-L25",), r"padding written: row 0 element 26 "),
    "idle piece rewritten in place through x * 1 + 0": (("uniform-first-piece-idle-col1-f32-L24",), r"\[in place\]: a level of plain COPY stages is no bit copy"),
    "mask byte of point p + 1": (("uniform-mask-on-one-piece-f64-L24",), r"NaN where numpy has none, or none where numpy has one"),
    "mask read although the stage does not use it": (("typed-float32-with-an-unused-mask-in-place",), r"NaN where numpy has none"),
    "parameter used in float64 and the result rounded": (("uniform-two-pieces-f32-L24",), r"values differ from numpy's bits"),
    "stage order swapped": (("levels-2-stages-f64-L25",), r"values differ from numpy's bits|NaN where numpy has none"),
    "17th sparse column aliased to the first": (("sparse-5-of-15-declines-f32",), r"sparse-5-of-15-declines-f32 \[in place\]: route sparse, the case is written for table"),
    "the float64 fields lane's second vector dropped": (("fields-f64-N32",), r"point 16: kernel np\.float64\(12345\.0\)"),
    "tail points dropped": (("fields-f32-N5",), r"point 4: kernel np\.float32\(12345\.0\)"),
    "tail points masked by vector index": (("fields-f32-N35",), r"fields-f32-N35 \[out of place\]: NaN where numpy has none, or none where numpy has one — level \d point 3[234]"),
    "the TRANS twin contracts AFFINE into an fma": (("levels-exp-log-f64",), r"values differ from numpy's bits"),
    "stages beyond the 4th ignored": ((f"fields-{SMALL.max_stages}-stages-f32",), r"values differ from numpy's bits|NaN where numpy has none"),
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
