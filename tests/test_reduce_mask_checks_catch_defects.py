"""The checks of tests/reduce_mask_checks.py, run on the CPU against a numpy stand-in of ``native.reduce`` / ``reduce_stack`` /
``mask_build`` / ``mask_count`` / ``mask_to_index`` / ``check_indices`` / ``stream_copy`` that reads the same pitched buffers and walks
them as the kernels do (items dealt to lanes, workgroups, sweeps; partials; a finish) — once as it is (every check passes) and once
per planted defect (the check that is there for it fails).  No deliberately broken kernel ever runs on a device.  The stand-in's
constants are small, so "past the cap" is a few hundred elements here; the checks take the constants as an argument for this."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import reduce_mask_checks as C
from anemoi_transform_amd import native

CPU = torch.device("cpu")
SMALL = C.Constants(block=8, wave=4, red_grid=4, red_unroll=2, stream_grid=8, per_lane=4, count_grid=4, self_scan=6)


class StandIn:
    def __init__(self, k: C.Constants = SMALL, defect: str | None = None):
        self.k, self.defect, self.workspace = k, defect, True
        self._maps = {}

    def kernels(self) -> C.Kernels:
        return C.Kernels(reduce=self.reduce, reduce_stack=self.reduce_stack, mask_build=self.mask_build, mask_count=self.mask_count,
                         mask_to_index=self.mask_to_index, index_into=self.index_into, check_indices=self.check_indices,
                         stream_copy=self.stream_copy, use_workspace=lambda flag: setattr(self, "workspace", flag))

    # ---- reductions: reduce_rows of csrc/atx_reduce.hip ---------------------------------------------------------------------
    def reduce(self, x, red, n=None):
        n = x.numel() if n is None else n
        return self._reduce_rows(x, 1, n, n, red)

    def reduce_stack(self, x, red, *, n_pts, n_lev, pitch, layout):
        if layout == native.COLUMNS:
            return self._reduce_rows(x, n_pts, n_lev, pitch, red)
        return self._reduce_rows(x, n_lev, n_pts, pitch, red)

    def _item_map(self, n_rows, row_len, pitch, vec, aligned):
        """(element offsets, their workgroup, their sweep, tail offsets, vector route?)"""
        key = (n_rows, row_len, pitch, vec, aligned)
        if key in self._maps:
            return self._maps[key]
        k = self.k
        tail = row_len % vec if n_rows == 1 else 0
        body = row_len - tail
        cols = -(-body // vec)
        vec_ok = aligned and (n_rows == 1 or (pitch % vec == 0 and cols * vec <= pitch))
        if vec_ok:
            read = cols * vec if (self.defect == "partial vector read whole" and n_rows > 1) else body
            r, c = np.divmod(np.arange(n_rows * read, dtype=np.int64), max(read, 1))
            item = r * cols + c // vec
            cap = k.red_grid - (1 if tail else 0)
        else:
            r, c = np.divmod(np.arange(n_rows * row_len, dtype=np.int64), max(row_len, 1))
            item = r * row_len + c
            cap, tail = k.red_grid, 0
        n_items = int(item.max()) + 1 if item.size else 0
        grid = min(cap, max(1, -(-n_items // (k.block * k.red_unroll))))
        stride = grid * k.block
        out = (r * pitch + c, (item % stride) // k.block, item // (stride * k.red_unroll), body + np.arange(tail), vec_ok, grid if n_items else 0)
        self._maps[key] = out
        return out

    def _partial(self, d):
        """(lo, hi, NaN count) of one workgroup's elements, as its lanes and its combine leave them."""
        big = np.finfo(np.float64).max if self.defect == "accumulators start at the largest finite value" else np.inf
        nans = int(np.isnan(d).sum())
        if nans:
            return math.nan, math.nan, nans
        return (min(big, float(d.min())), max(-big, float(d.max())), 0) if d.size else (big, -big, 0)

    def _finish(self, parts, is_max):
        """reduce_final_kernel / the atomics: NaN wins."""
        ident = -math.inf if is_max else math.inf
        if not parts:
            return ident
        a = np.array(parts, dtype=np.float64)
        if self.defect == "a clean partial wins the finish":
            return float(np.fmax.reduce(a) if is_max else np.fmin.reduce(a))
        return float(np.max(a) if is_max else np.min(a))

    def _reduce_rows(self, x, n_rows, row_len, pitch, red):
        assert pitch >= row_len
        a = x.numpy().reshape(-1) if x.numel() else np.zeros(0, dtype=np.float32 if x.dtype == torch.float32 else np.float64)
        vec = 4 if x.dtype == torch.float32 else 2
        if n_rows == 0 or row_len == 0:
            lo, hi, cnt = math.inf, -math.inf, 0.0
        else:
            off, wg, sweep, tail_off, vec_ok, grid = self._item_map(n_rows, row_len, pitch, vec, x.data_ptr() % 16 == 0)
            if self.defect == "only the first sweep":
                keep = sweep == 0
                off, wg = off[keep], wg[keep]
            d = a[off].astype(np.float64)
            parts = [self._partial(d[wg == g]) for g in range(grid)]
            if tail_off.size and self.defect != "tail dropped":
                parts.append(self._partial(a[tail_off].astype(np.float64)))
            los, his = [p[0] for p in parts], [p[1] for p in parts]
            if self.defect == "second pass reads the first pass's partials" and not vec_ok and self.workspace and red == native.RED_MINMAX:
                his = los
            lo, hi, cnt = self._finish(los, False), self._finish(his, True), float(sum(p[2] for p in parts))
        if red == native.RED_MINMAX:
            return lo, hi
        return {native.RED_MIN: lo, native.RED_MAX: hi, native.RED_NANCOUNT: cnt}[red]

    # ---- masks --------------------------------------------------------------------------------------------------------------
    def mask_build(self, m, mask, *, n, stride=1, cmp, threshold=0.0):
        assert mask.dtype == torch.uint8 and mask.data_ptr() % 4 == 0
        if n == 0:
            return
        if self.defect == "m_stride ignored":
            stride = 1
        v = m.numpy().reshape(-1)[: (n - 1) * stride + 1: stride]
        op = {c: name for name, c in C.CMPS.items()}[cmp]
        with np.errstate(all="ignore"):
            if op == "NOTNAN":
                res = ~np.isnan(v)
            elif op == "ISNAN":
                res = np.isnan(v)
            elif self.defect == "float32 compared in float64":
                res = C.UFUNCS[op](v.astype(np.float64), np.float64(threshold))
            else:
                res = C.UFUNCS[op](v, v.dtype.type(threshold))  # (float)threshold
            if op == "NE" and self.defect == "NE false for NaN":
                res = res & ~np.isnan(v)
        written = n - n % 4 if self.defect == "n % 4 tail skipped" else n
        mask.numpy()[:written] = res[:written]

    def mask_count(self, mask, n=None):
        n = mask.numel() if n is None else n
        b = mask.numpy()[:n]
        return int(b.sum(dtype=np.int64)) if self.defect == "mask_count sums byte values" else int(np.count_nonzero(b))

    def index_into(self, mask, n, index):
        """compact_count + compact_scatter: every kChunk bytes write their positions from the count of the chunks before them."""
        b, out, chunk = mask.numpy()[:n], index.numpy(), self.k.chunk
        before = 0
        for c0 in range(0, n, chunk):
            idx = c0 + np.flatnonzero(b[c0: c0 + chunk])
            at = before - 1 if (self.defect == "offset off by one at a kChunk boundary" and c0 > 0 and before > 0) else before
            out[at: at + idx.size] = idx
            before += idx.size
        if self.defect == "writes one past count" and before > 0:
            out[before] = out[before - 1]
        return before

    def mask_to_index(self, mask, n=None):
        n = mask.numel() if n is None else n
        index = torch.empty(max(n, 1) + 1, dtype=torch.int32)
        return index[: self.index_into(mask, n, index)]

    def check_indices(self, idx, n_src):
        t = idx.numpy().astype(np.int64)
        return int(((t < 0) | ((t > n_src) if self.defect == "check_indices accepts n_src" else (t >= n_src))).sum())

    def stream_copy(self, src, dst):
        dst.numpy().view(np.uint8)[...] = src.numpy().view(np.uint8)


# ---- the runs ---------------------------------------------------------------------------------------------------------------
def shapes_named(part: str, k=SMALL):
    every = [s for dt in C.DTYPES for s in C.small_shapes(dt) + C.mid_shapes(dt, k) + C.flat_shapes(dt, k)]
    return [s for s in every if part in s.name]


def run_reduce_checks(kern, shapes, k=SMALL, walked=True, special=True):
    for s in shapes:
        if walked:
            assert C.check_walked_positions(kern, CPU, s, k) > 0
        if special:
            C.check_special_values(kern, CPU, s)


def run_past_the_cap(kern, k=SMALL, only=None):
    sizes = []
    for s, host_copy in C.past_cap_shapes(k):
        if only is None or only in s.name:
            sizes.append(C.check_past_the_cap(kern, CPU, s, k, host_copy=host_copy))
    return sizes


def run_mask_checks(kern, k=SMALL, build=True, index=True):
    if build:
        for dt in C.DTYPES:
            for thr in C.THRESHOLDS:
                C.check_mask_build(kern, CPU, dt, thr, k)
            assert C.check_mask_build_past_the_cap(kern, CPU, dt, k) > k.stream_grid * k.block * 4
    if index:
        for n in C.index_lengths(k):
            for density in C.DENSITIES:
                C.check_mask_count_and_index(kern, CPU, n, density)


def run_guard_checks(kern, k=SMALL):
    for n in C.check_indices_lengths(k):
        C.check_check_indices(kern, CPU, n, k)
    for n_bytes in C.stream_copy_sizes(k):
        C.check_stream_copy(kern, CPU, n_bytes)


def test_the_stand_in_passes_every_check():
    kern = StandIn().kernels()
    run_reduce_checks(kern, shapes_named(""))
    sizes = run_past_the_cap(kern)
    assert {z["route"] for z in sizes} == {"16-byte", "scalar"} and all(z["items"] > 2 * z["threshold"] for z in sizes)
    run_mask_checks(kern)
    run_guard_checks(kern)


# defect -> (what to run, the assertion that catches it)
DEFECTS = {
    "partial vector read whole": (lambda k: run_reduce_checks(k, shapes_named("f32-columns-len5-wide16-nan"), special=False), r"walked extreme: .*constant field"),
    "tail dropped": (lambda k: run_reduce_checks(k, shapes_named("f32-flat-7"), special=False), r"walked extreme: .*the minimum at the last element of the first row \(row 0, col 6\)"),
    "only the first sweep": (lambda k: run_past_the_cap(k, only="f64-fields"), r"past the cap: .*closed form"),
    "a clean partial wins the finish": (lambda k: run_reduce_checks(k, shapes_named("f64-columns-137"), special=False), r"walked NaN: .*kernel \(?[0-9]"),
    "second pass reads the first pass's partials": (lambda k: run_reduce_checks(k, shapes_named("f32-columns-137x"), special=False),
                                                    r"walked extreme: .*\[scalar route, workspace\] MINMAX"),
    "accumulators start at the largest finite value": (lambda k: run_reduce_checks(k, shapes_named("f64-fields-len3-tight"), walked=False), r"special values: .*all \+inf"),
    "float32 compared in float64": (lambda k: run_mask_checks(k, index=False), r"mask_build: float32 .* 0\.1, "),
    "NE false for NaN": (lambda k: run_mask_checks(k, index=False), r"mask_build: float32 NE "),
    "n % 4 tail skipped": (lambda k: run_mask_checks(k, index=False), r"mask_build: .*n = 1, .*differ from numpy"),
    "m_stride ignored": (lambda k: run_mask_checks(k, index=False), r"mask_build: stride: .*m_stride = 3"),
    "mask_count sums byte values": (lambda k: run_mask_checks(k, build=False), r"mask_count: "),
    "offset off by one at a kChunk boundary": (lambda k: run_mask_checks(k, build=False), r"index list: n = 33, .*differs from np.flatnonzero"),
    "writes one past count": (lambda k: run_mask_checks(k, build=False), r"written past index\[count\)"),
    "check_indices accepts n_src": (lambda k: run_guard_checks(k), r"check_indices: .* 1000 at 0: kernel 0, numpy 1"),
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_check_catches_its_defect(defect):
    run, message = DEFECTS[defect]
    with pytest.raises(AssertionError, match=message):
        run(StandIn(defect=defect).kernels())


def test_the_checks_run_every_route_past_the_real_cap():
    """The sizes the GPU module runs, from the kernels' own constants: every shape has more than two sweeps of the capped grid on
    its route, both routes and a tail of 1 and of 3 are there, and nothing is larger than the module's 4 GB."""
    k = C.K
    assert k.sweep_items() == k.red_grid * k.block * k.red_unroll and k.sweep_items(True) == (k.red_grid - 1) * k.block * k.red_unroll
    shapes = [s for s, _ in C.past_cap_shapes(k)]
    for s in shapes:
        beyond = s.n_items() - k.sweep_items(s.tail > 0)
        assert beyond >= k.sweep_items(s.tail > 0) + 1 and beyond % 2 == 1, s.name
        assert (s.n_rows * s.pitch + 16) * np.dtype(s.np_dtype).itemsize < 4 << 30
    for dt in C.DTYPES:
        mine = [s for s in shapes if s.np_dtype == dt]
        assert {(s.kind, s.route()) for s in mine} == {(kind, r) for kind in ("flat", "columns", "fields") for r in ("16-byte", "scalar")}
    assert sorted(s.tail for s in shapes if s.tail) == [1, 1, 3]
    assert sum(host for _, host in C.past_cap_shapes(k)) == 2


def test_numpy_compares_a_float32_field_in_float32():
    """What reduce_mask_checks' docstring records: ``float32_array > 0.1`` is the float32 comparison against ``np.float32(0.1)`` —
    the kernel's ``(float)threshold`` — and not the float64 one, which differs where the field holds ``np.float32(0.1)``."""
    a = np.array([np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(1)), np.nextafter(np.float32(0.1), np.float32(0)), 0.0], dtype=np.float32)
    assert np.array_equal(a > 0.1, a > np.float32(0.1)) and np.array_equal(a >= 0.1, a >= np.float32(0.1))
    assert np.array_equal(a > 0.1, [False, True, False, False])
    assert np.array_equal(a.astype(np.float64) > 0.1, [True, True, False, False])
    assert np.array_equal(C.mask_reference(a, "GT", 0.1), a > 0.1) and np.array_equal(C.mask_reference(a, "EQ", 0.1), a == 0.1)
