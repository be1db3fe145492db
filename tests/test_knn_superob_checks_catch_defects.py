"""The checks of tests/knn_superob_checks.py, run on the CPU against a numpy stand-in of ``native.KnnIndex``, ``native.cutout_inside``,
``native.obs_group_mean`` and ``native.obs_group_argmin`` that walks the buffers as the kernels do (Morton order, leaves of kLeaf points, a
box tree walked with a stack and pruned by the k-th best; one triangle per neighbour rotation; a lane per group, a wave per long
group) — once as it is (every check passes) and once per planted defect (the named case fails).  No deliberately broken kernel ever
runs on a device."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import knn_superob_checks as C

CPU = torch.device("cpu")
K = C.K
INT32_MAX = 2**31 - 1


# ---- k-NN: csrc/atx_knn.hip restated ------------------------------------------------------------------------------------------
def spread21(v: np.ndarray) -> np.ndarray:
    v = v & np.uint64(0x1FFFFF)
    for shift, mask in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(shift))) & np.uint64(mask)
    return v


class StandInIndex:
    def __init__(self, owner: "StandIn", src: torch.Tensor, workspace):
        self.owner, self.k = owner, owner.k
        self.src = src.numpy()
        self.n_src = len(self.src)
        self.workspace = workspace
        leaf = self.k.leaf
        with np.errstate(all="ignore"):
            v = np.clip((self.src + 1.0) * 0.5, 0.0, 1.0)
            v = np.where(np.isnan(v), 0.0, v)
        q = (v * 2097151.0).astype(np.uint64)
        keys = spread21(q[:, 0]) | (spread21(q[:, 1]) << np.uint64(1)) | (spread21(q[:, 2]) << np.uint64(2))
        self.order = np.argsort(keys, kind="stable").astype(np.int32)
        self.sorted = self.src[self.order]
        n_leaves = -(-self.n_src // leaf)
        self.n_pow2 = 1 << max(0, (n_leaves - 1).bit_length())
        self.boxes = np.empty((2 * self.n_pow2, 6))
        self.boxes[:, :3], self.boxes[:, 3:] = np.inf, -np.inf
        for j in range(n_leaves):
            p = self.sorted[j * leaf: min(self.n_src, (j + 1) * leaf)]
            self.boxes[self.n_pow2 + j, :3], self.boxes[self.n_pow2 + j, 3:] = p.min(axis=0), p.max(axis=0)
        for node in range(self.n_pow2 - 1, 0, -1):
            a, c = self.boxes[2 * node], self.boxes[2 * node + 1]
            self.boxes[node, :3], self.boxes[node, 3:] = np.minimum(a[:3], c[:3]), np.maximum(a[3:], c[3:])

    def box_dist2(self, node: int, x) -> float:
        b = self.boxes[node]
        s = 0.0
        for d in range(3):
            t = 0.0
            if x[d] < b[d]:
                t = x[d] - b[d]
            elif x[d] > b[3 + d]:
                t = x[d] - b[3 + d]
            s = s + t * t
        return s

    def query(self, tgt: torch.Tensor, k: int, out=None):
        defect, leaf = self.owner.defect, self.k.leaf
        assert 1 <= k <= self.k.max_k
        self.owner.instances.add(k)
        tg = tgt.numpy()
        n = len(tg)
        idx, d2 = np.empty((n, k), np.int32), np.empty((n, k))
        higher = defect == "ties ordered by the higher index"

        def before(cd, ci, bd, bi):
            return cd < bd or (cd == bd and (ci > bi if higher and bi != INT32_MAX else ci < bi))

        for t in range(n):
            x = tg[t].tolist()
            best_d, best_i = [math.inf] * k, [INT32_MAX] * k
            stack = [1]
            while stack:
                node = stack.pop()
                worst = best_d[k - 2] if (defect == "the bound taken from the (k-1)-th entry" and k >= 2) else best_d[k - 1]
                bd = self.box_dist2(node, x)
                if bd >= worst if defect == "pruning with >=" else bd > worst:
                    continue
                if node >= self.n_pow2:
                    p0 = (node - self.n_pow2) * leaf
                    p1 = min(self.n_src, p0 + leaf)
                    if defect == "the last partial leaf dropped" and p0 + leaf > self.n_src:
                        continue
                    pts = self.sorted[p0:p1]
                    dx, dy, dz = pts[:, 0] - x[0], pts[:, 1] - x[1], pts[:, 2] - x[2]
                    if defect == "distance summed in another order":
                        s = (0.0 + dz * dz + dy * dy) + dx * dx
                    else:
                        s = ((0.0 + dx * dx) + dy * dy) + dz * dz
                    for cd, ci in zip(s.tolist(), self.order[p0:p1].tolist()):
                        if before(cd, ci, best_d[k - 1], best_i[k - 1]):
                            for j in range(k):
                                if before(cd, ci, best_d[j], best_i[j]):
                                    best_d[j], cd = cd, best_d[j]
                                    best_i[j], ci = ci, best_i[j]
                else:
                    l, r = 2 * node, 2 * node + 1
                    dl, dr = self.box_dist2(l, x), self.box_dist2(r, x)
                    strict = defect == "pruning with >="
                    keep_l, keep_r = (dl < worst if strict else dl <= worst), (dr < worst if strict else dr <= worst)
                    if dl <= dr:
                        stack += ([r] if keep_r else []) + ([l] if keep_l else [])
                    else:
                        stack += ([l] if keep_l else []) + ([r] if keep_r else [])
            missing = -1 if defect == "the not-found marker -1" else self.n_src
            idx[t] = [missing if i == INT32_MAX else i for i in best_i]
            d2[t] = best_d
        if out is None:
            return torch.from_numpy(idx), torch.from_numpy(d2)
        out[0].numpy()[...] = idx
        out[1].numpy()[...] = d2
        return out


# ---- the stand-in ---------------------------------------------------------------------------------------------------------------
class StandIn:
    def __init__(self, defect: str | None = None, k: C.Constants = K):
        self.defect, self.k = defect, k
        self.instances = set()

    def kernels(self) -> C.Kernels:
        return C.Kernels(knn_build=lambda src, workspace=None: StandInIndex(self, src, workspace),
                         knn_workspace_bytes=lambda n: (1 + -(-n * 64 // 256)) * 256,
                         cutout_inside=self.cutout_inside, group_mean=self.group_mean, group_argmin=self.group_argmin)

    # ---- cutout_inside_kernel -------------------------------------------------------------------------------------------------
    def dot3(self, a, b):
        if self.defect == "a dot with two roundings per term":
            return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
        return C.dot3(a, b)

    def cutout_inside(self, g, lam, nb, out=None):
        n, k = nb.shape
        n_lam = lam.shape[0]
        gh, lh, flat = g.numpy(), lam.numpy(), nb.numpy().reshape(-1)
        res = out.numpy() if out is not None else np.zeros(n, np.uint8)
        eps = C.EPSILON
        for i in range(n):
            d = gh[i].tolist()
            hit = False
            for j in range(k):
                if self.defect == "the triangle rotation without the wrap":
                    tri = [int(flat[min(i * k + j + m, flat.size - 1)]) for m in range(3)]
                else:
                    tri = [int(flat[i * k + (j + m) % k]) for m in range(3)]
                if any(t < 0 or t >= n_lam for t in tri):
                    if self.defect != "a stray index read as row 0":
                        continue
                    tri = [t if 0 <= t < n_lam else 0 for t in tri]
                v0, v1, v2 = (lh[t].tolist() for t in tri)
                e1, e2, s = [v1[c] - v0[c] for c in range(3)], [v2[c] - v0[c] for c in range(3)], [0.0 - v0[c] for c in range(3)]
                h = C.cross3(d, e2)
                a = self.dot3(e1, h)
                if -eps < a < eps:
                    continue
                f = 1.0 / a
                u = f * self.dot3(s, h)
                if (u <= 0.0 if self.defect == "u <= 0 rejected" else u < 0.0) or u > 1.0:
                    continue
                q = C.cross3(s, e1)
                v = f * self.dot3(d, q)
                if v < 0.0 or u + v > 1.0:
                    continue
                if f * self.dot3(e2, q) > eps:
                    hit = True
                    break
            res[i] = 1 if hit else 0
        return torch.from_numpy(res) if out is None else out

    # ---- obs_group_mean_kernel ------------------------------------------------------------------------------------------------
    def kahan(self, values):
        """(sum, n) of the kernel's Kahan struct over ``values`` in order."""
        total = comp = 0.0
        n = 0
        for v in values:
            if v != v:
                if self.defect == "NaN counted in the divisor":
                    n += 1
                continue
            y = v - comp
            t = total + y
            comp = (t - total) - y
            if comp != comp and self.defect != "the compensation not reset after inf":
                comp = 0.0
            total = t
            n += 1
        return total, n

    def segment(self, offsets, g, n_groups, n_sel):
        if g >= n_groups:
            return None
        b, e = int(offsets[g]), int(offsets[g + 1])
        return None if (b < 0 or e < b or e > n_sel) else (b, e)

    @staticmethod
    def rows_of(col, order, b, e):
        """superob_value over positions b .. e: a row index outside the column reads as NaN."""
        r = order[b:e].astype(np.int64)
        ok = (r >= 0) & (r < len(col))
        out = np.full(e - b, np.nan)
        out[ok] = col[r[ok]]
        return out.tolist()

    def group_mean(self, values, order, offsets, mean, count):
        k, n_cols = self.k, values.shape[0]
        n_sel, n_groups = order.numel(), offsets.numel() - 1
        vh, oh, fh = values.numpy(), order.numpy(), offsets.numpy()
        out_pitch = mean.stride(0) if n_cols > 1 else max(n_groups, 1)
        if n_cols > 1:
            assert count.stride(0) == out_pitch
        if self.defect == "the output pitch ignored":
            out_pitch = max(n_groups, 1)
        # the outputs as the kernel addresses them: flat from the first element, rows out_pitch apart
        span = (n_cols - 1) * max(mean.stride(0), out_pitch) + n_groups if n_groups else 0
        mflat = torch.as_strided(mean, (span,), (1,)).numpy() if span else None
        cflat = torch.as_strided(count, (span,), (1,)).numpy() if span else None
        for c in range(n_cols):
            col = vh[c]
            for w0 in range(0, n_groups, k.wave):
                acc = {}
                long_lanes = []
                for lane in range(k.wave):
                    g = w0 + lane
                    seg = self.segment(fh, g, n_groups, n_sel)
                    acc[lane] = (0.0, 0)
                    if seg is None:
                        continue
                    b, e = seg
                    if e - b >= k.long_group:
                        long_lanes.append((lane, b, e))
                        continue
                    if self.defect == "the tail after the last multiple of the unroll dropped":
                        e = b + (e - b) // k.unroll * k.unroll
                    acc[lane] = self.kahan(self.rows_of(col, oh, b, e))
                for lane, b, e in long_lanes:
                    if self.defect == "the last partial block of a wave dropped in a long group":
                        e = b + (e - b) // k.wave * k.wave
                    vals = self.rows_of(col, oh, b, e)
                    if self.defect == "long groups summed from per-lane partials":
                        total, n = 0.0, 0
                        for j in range(k.wave):
                            s, m = self.kahan(vals[j::k.wave])
                            total, n = total + s, n + m
                        wide = (total, n)
                    else:
                        wide = self.kahan(vals)
                    to = (lane + 1) % k.wave if self.defect == "a long group's result written by the wrong lane" else lane
                    acc[to] = wide
                for lane in range(k.wave):
                    g = w0 + lane
                    if g < n_groups:
                        s, n = acc[lane]
                        with np.errstate(all="ignore"):
                            mflat[c * out_pitch + g] = np.float64(s) / np.float64(n) if n > 0 else np.nan
                        cflat[c * out_pitch + g] = n

    # ---- obs_group_argmin_kernel ----------------------------------------------------------------------------------------------
    def see(self, best, v, at):
        d, k = best
        if self.defect == "the last of equals taken":
            take = v <= d or (k is None and v == v)
        elif self.defect == "NaN beats numbers":
            take = v < d or k is None
        else:
            take = v < d or (k is None and v == v)
        return (v, at) if take else best

    def group_argmin(self, distance, order, offsets, nearest):
        k = self.k
        n_obs, n_sel, n_groups = distance.numel(), order.numel(), offsets.numel() - 1
        dh, oh, fh, out = distance.numpy(), order.numpy(), offsets.numpy(), nearest.numpy()
        for g in range(n_groups):
            seg = self.segment(fh, g, n_groups, n_sel)
            best = (math.inf, None)
            if seg is not None:
                b, e = seg
                vals = self.rows_of(dh, oh, b, e)
                if e - b < k.long_group:
                    for j, v in enumerate(vals):
                        best = self.see(best, v, b + j)
                else:
                    lanes = []
                    for lane in range(k.wave):
                        mine = (math.inf, None)
                        for j in range(lane, e - b, k.wave):
                            mine = self.see(mine, vals[j], b + j)
                        lanes.append(mine)
                    for d, at in lanes:  # the butterfly's result: the smallest (distance, position)
                        if at is None:
                            continue
                        if self.defect == "the merge ignores position":
                            better = best[1] is None or d < best[0]
                        else:
                            better = best[1] is None or d < best[0] or (d == best[0] and at < best[1])
                        if better:
                            best = (d, at)
            at = best[1]
            if at is None:
                at = seg[0] if (seg is not None and seg[1] > seg[0] and self.defect != "an all-NaN group gives -1") else -1
            r = int(oh[at]) if at >= 0 else -1
            out[g] = r if 0 <= r < n_obs else -1


# ---- the runs -------------------------------------------------------------------------------------------------------------------
SMALL = C.Constants(leaf=K.leaf, max_k=K.max_k, unroll=K.unroll, long_group=K.long_group, block=8, wave=K.wave, build_grid=4)


def run_knn(kern, every_k=True, sizes=True, targets=True, ties=True, reuse=True, buffers=True, past_cap=True):
    if every_k:
        C.check_knn_every_k(kern, CPU)
    if sizes:
        for n_src in C.knn_source_sizes():
            C.check_knn_source_size(kern, CPU, n_src)
    if targets:
        for n_tgt in C.knn_target_counts():
            C.check_knn_target_count(kern, CPU, n_tgt)
    if ties:
        for name in C.tie_sets():
            C.check_knn_ties(kern, CPU, name)
    if reuse:
        C.check_knn_reuse(kern, CPU)
    if buffers:
        C.check_knn_buffers(kern, CPU)
    if past_cap:
        C.check_knn_past_the_cap(kern, CPU, SMALL)  # a few hundred points here; the device module takes the kernels' own cap


def only_knn(**which):
    flags = dict(every_k=False, sizes=False, targets=False, ties=False, reuse=False, buffers=False, past_cap=False)
    flags.update(which)
    return lambda kern: run_knn(kern, **flags)


def run_cutout(kern, patch=True, constructed=True, epsilon=True, stray=True, edges=True):
    if edges:
        C.check_cutout_edge_points(kern, CPU)
    if patch:
        for k, n in C.CUTOUT_SHAPES:
            C.check_cutout_patch(kern, CPU, k, n)
    if constructed:
        C.check_cutout_constructed(kern, CPU)
    if epsilon:
        C.check_cutout_epsilon(kern, CPU)
    if stray:
        C.check_cutout_stray(kern, CPU)


def run_mean(kern, lengths=True, counts=True, special=True, guards=True):
    if lengths:
        for shuffled in (False, True):
            C.check_mean_edge_lengths(kern, CPU, shuffled)
    if counts:
        for name in C.group_count_cases():
            C.check_mean_group_counts(kern, CPU, name)
    if special:
        C.check_mean_special_values(kern, CPU)
    if guards:
        C.check_superob_guards(kern, CPU)


def run_argmin(kern, walk=True, edges=True):
    if walk:
        for length in (K.long_group + K.wave + 1, K.long_group):
            C.check_argmin_walk(kern, CPU, length)
    if edges:
        C.check_argmin_edge_groups(kern, CPU)


def test_the_stand_in_passes_every_check_and_every_instance_is_requested():
    stand_in = StandIn()
    kern = stand_in.kernels()
    run_knn(kern)
    assert stand_in.instances == set(range(1, K.max_k + 1)), f"template instances requested: {sorted(stand_in.instances)}"
    run_cutout(kern)
    run_mean(kern)
    run_argmin(kern)


def test_every_instance_is_requested_by_the_neighbour_count_case_alone():
    stand_in = StandIn()
    C.check_knn_every_k(stand_in.kernels(), CPU)
    assert stand_in.instances == set(range(1, K.max_k + 1))


# defect -> (what to run, the assertion of the named case that catches it)
DEFECTS = {
    # k-NN
    "ties ordered by the higher index": (only_knn(ties=True), r"k-NN: ties: 100 coincident sources: .* k = 1: .*indices differ"),
    "pruning with >=": (only_knn(ties=True), r"k-NN: ties: .*indices differ"),
    "the last partial leaf dropped": (only_knn(sizes=True), r"k-NN: source sizes: n_src = 1, .*differ"),
    "the bound taken from the (k-1)-th entry": (only_knn(every_k=True), r"k-NN: every neighbour count: .* k = 2: .*differ"),
    "the not-found marker -1": (only_knn(sizes=True), r"k-NN: source sizes: n_src = 1, .* k = 2: .*indices differ"),
    "distance summed in another order": (only_knn(targets=True), r"k-NN: target counts: .*(squared distances differ in bits|indices differ)"),
    # cutout
    "a dot with two roundings per term": (lambda k: run_cutout(k, patch=False, constructed=False, epsilon=False, stray=False), r"cutout: points on the edges of a regular patch: .*differ from the reference"),
    "u <= 0 rejected": (lambda k: run_cutout(k, patch=False, epsilon=False, stray=False, edges=False), r"cutout: constructed: .*rotation \(0, 1, 2\) alone: .*points differ from the reference, first at \[0"),
    "a stray index read as row 0": (lambda k: run_cutout(k, patch=False, constructed=False, epsilon=False, edges=False), r"cutout: stray indices -1 and n_lam: .*differ from the reference"),
    "the triangle rotation without the wrap": (lambda k: run_cutout(k, constructed=False, epsilon=False, stray=False, edges=False), r"cutout: neighbour tables of a jittered patch: n = \d+, k = \d+, .*differ"),
    # mean
    "long groups summed from per-lane partials": (lambda k: run_mean(k, counts=False, special=False, guards=False), r"group mean: edge lengths in order: .*means differ in bits"),
    "the tail after the last multiple of the unroll dropped": (lambda k: run_mean(k, counts=False, special=False, guards=False), r"group mean: edge lengths in order: .*differ"),
    "the last partial block of a wave dropped in a long group": (lambda k: run_mean(k, counts=False, special=False, guards=False), r"group mean: edge lengths in order: .*differ"),
    "NaN counted in the divisor": (lambda k: run_mean(k, lengths=False, counts=False, guards=False), r"group mean: special values: .*differ"),
    "the compensation not reset after inf": (lambda k: run_mean(k, lengths=False, counts=False, guards=False), r"group mean: special values: .*means differ in bits"),
    "a long group's result written by the wrong lane": (lambda k: run_mean(k, lengths=False, special=False, guards=False), r"group mean: \d+ groups, long at .*differ"),
    "the output pitch ignored": (lambda k: run_mean(k, counts=False, special=False, guards=False), r"group mean: edge lengths in order: .*out_pitch = 23: .*differ"),
    # argmin
    "the last of equals taken": (lambda k: run_argmin(k, walk=False), r"group argmin: edge groups: .*differ from the row-order loop, first \[0"),
    "the merge ignores position": (lambda k: run_argmin(k, walk=False), r"group argmin: edge groups: .*differ from the row-order loop"),
    "NaN beats numbers": (lambda k: run_argmin(k, walk=False), r"group argmin: edge groups: .*differ from the row-order loop"),
    "an all-NaN group gives -1": (lambda k: run_argmin(k, walk=False), r"group argmin: edge groups: .*kernel \[-1"),
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_named_case_catches_its_defect(defect):
    run, message = DEFECTS[defect]
    with pytest.raises(AssertionError, match=message) as caught:
        run(StandIn(defect=defect).kernels())
    print(f"{defect}: {str(caught.value)[:300]}")


def test_the_edge_sizes_come_from_the_kernels_constants():
    """What the device module runs: the group lengths and counts of the issue at today's constants, and the past-the-cap size."""
    assert (K.leaf, K.max_k, K.unroll, K.long_group, K.block, K.wave, K.build_grid) == (8, 17, 8, 256, 256, 64, 4096)
    assert C.edge_lengths() == [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 1000]
    assert sorted({len(v[0]) for v in C.group_count_cases().values()}) == [1, 63, 64, 65, 255, 256, 257, 513]
    assert K.past_cap_sources() == 16 * 2**20 + 9 and K.build_sweep == 2**20
    assert set(C.knn_source_sizes()) == {1, 2, 7, 8, 9, 15, 17, 63, 64, 65, 511, 513}
    assert any(n < k for n in C.knn_source_sizes() for k in C.knn_size_ks(n))
    assert C.knn_target_counts() == [1, 63, 64, 65, 255, 256, 257]
    assert list(C.knn_every_k()) == list(range(1, 18))
    assert {k for k, _ in C.CUTOUT_SHAPES} == {1, 2, 3, 4, 5, 17} and {n for _, n in C.CUTOUT_SHAPES} >= {0, 1, 255, 256, 257}
