"""rotate_winds / unrotate_winds: vector components between projection frames (R: filters/fields/rotate_winds.py).

The reference rotates each (x_wind, y_wind) pair with ``earthkit.geo.rotate.rotate_vector`` on the host, pair by pair.  Here
the frame of every grid point is built once per grid and projection pair on the host (``projections.vector_frame``, float64)
and kept in HBM on the filter; the pairs on one grid go to ONE ``atx_rotate_vectors_stack`` launch, operand ``i`` of every pair
becoming level ``g`` of one stack.  Pairs are grouped by grid IDENTITY (the coordinate hash the k-NN cache keys its tables
by) and projection pair, not by grid size as ``combine_groups`` does: the frame depends on where the points are.
"""

from __future__ import annotations

import logging
from typing import Any, Iterator

import numpy as np
import torch

from .. import native
from ..core import filter_registry
from ..fields import FieldList, fields_to_stack, new_field_from_stack
from ..interp import points_hash
from ..projections import parse, vector_frame
from ..stack import Stack
from .multi import MatchingFieldsFilter, MatchingSpec

LOG = logging.getLogger(__name__)

_KIND = {"rotation": native.FRAME_ROTATION, "general": native.FRAME_GENERAL}


class RotateWinds(MatchingFieldsFilter):
    """Rotate wind components from one projection's frame to another's (R: rotate_winds.py:21-118)."""

    MATCHING = MatchingSpec(select="param", forward=("x_wind", "y_wind"), backward=("x_wind", "y_wind"))
    PARITY_NOTE = ("pyproj and earthkit-geo are restated (projections.py): eqc <-> longlat, the projection of a regular lat/lon "
                   "field, is pinned by the reference's literals at np.allclose; ob_tran / lcc / stere / merc are restated from "
                   "their spherical forward formulas and are NOT pinned against pyproj / earthkit-geo")

    def __init__(self, *, x_wind: str, y_wind: str, source_projection: str | None = None,
                 target_projection: str = "+proj=longlat") -> None:
        self.x_wind = x_wind
        self.y_wind = y_wind
        self.source_projection = source_projection
        self.target_projection = target_projection
        # (grid hash, source key, target key, dtype, device) -> (atx_frame kind, device table [n_pts, F])
        self._frames: dict[tuple, tuple[int, torch.Tensor]] = {}
        super().__init__()

    # ---- the projections of one pair ---------------------------------------------------------------------------------------
    def _projections(self, direction: str, x_wind: Any) -> tuple[str, str]:
        if direction == "backward":
            assert self.source_projection is not None, "source_projection cannot be None when unrotating winds!"
            return self.target_projection, self.source_projection
        if self.source_projection is not None:
            return self.source_projection, self.target_projection
        projection = x_wind.projection() if hasattr(x_wind, "projection") else None
        if projection is None:
            raise ValueError(f"rotate_winds: field {x_wind.metadata('param')!r} carries no projection; give source_projection=... "
                             "(a PROJ string)")
        return str(projection), self.target_projection

    def _frame(self, grid: str, lat: np.ndarray, lon: np.ndarray, src, tgt, dtype: torch.dtype, dev) -> tuple[int, torch.Tensor]:
        key = (grid, src.key, tgt.key, dtype, str(dev))
        if key not in self._frames:
            kind, table = vector_frame(lat, lon, src, tgt)
            self._frames[key] = (_KIND[kind], torch.from_numpy(np.ascontiguousarray(table)).to(device=dev, dtype=dtype))
        return self._frames[key]

    # ---- all pairs, one launch per grid and projection pair -----------------------------------------------------------------
    def _rotate(self, groups: list[tuple[Any, Any]], direction: str) -> list[tuple[tuple[Stack, int], tuple[Stack, int]]]:
        buckets: dict[tuple, list[int]] = {}
        # (lat, lon, content hash) of the coordinate arrays met so far: fields usually share their grid's arrays, and holding the
        # arrays (compared by identity) keeps an id from being reused by another grid's array within this call
        grids: list[tuple[np.ndarray, np.ndarray, str]] = []
        where: dict[tuple, tuple[str, np.ndarray, np.ndarray, Any, Any]] = {}
        for gi, (x, _) in enumerate(groups):
            src, tgt = (parse(p) for p in self._projections(direction, x))
            lat, lon = x.grid_points()
            grid = next((h for a, b, h in grids if a is lat and b is lon), None)
            if grid is None:
                grid = points_hash(lat, lon)
                grids.append((lat, lon, grid))
            key = (grid, src.key, tgt.key)
            buckets.setdefault(key, []).append(gi)
            where.setdefault(key, (grid, lat, lon, src, tgt))
        results: list[Any] = [None] * len(groups)
        for key, members in buckets.items():
            grid, lat, lon, src, tgt = where[key]
            xs = fields_to_stack([groups[gi][0] for gi in members])
            ys = fields_to_stack([groups[gi][1] for gi in members])
            assert xs.n_pts == ys.n_pts == len(lat), "x_wind and y_wind must share the grid of x_wind"
            dtype = torch.float32 if xs.dtype == ys.dtype == torch.float32 else torch.float64
            xs, ys = (s if s.dtype == dtype else Stack(s.data.to(dtype), s.n_pts, s.n_lev, s.layout) for s in (xs, ys))
            if ys.layout != xs.layout or ys.pitch != xs.pitch:  # one stack may be a whole resident stack of another pitch
                packed = xs.new_like()
                native.relayout(ys.data, packed.data, n_pts=ys.n_pts, n_lev=ys.n_lev, src_pitch=ys.pitch, dst_pitch=packed.pitch,
                                src_layout=ys.layout, dst_layout=packed.layout)
                ys = packed
            kind, frame = self._frame(grid, lat, lon, src, tgt, dtype, xs.device)
            xo, yo = xs.new_like(), ys.new_like()
            native.rotate_vectors_stack(xs.data, ys.data, xo.data, yo.data, frame, kind, n_pts=xs.n_pts, n_lev=xs.n_lev,
                                        pitch=xs.pitch, layout=xs.layout)
            for level, gi in enumerate(members):
                results[gi] = ((xo, level), (yo, level))
        return results

    def _run(self, data: Any, direction: str) -> FieldList:
        group_by = (self.x_wind, self.y_wind)
        data = data if isinstance(data, FieldList) else FieldList(list(data))
        self._check_metadata_match(set(data.metadata(self.MATCHING.select)), group_by)
        result: list[Any] = []
        groups = list(self._grouping(group_by).iterate(data, other=result.append))
        if groups:
            for (x, y), out in zip(groups, self._rotate(groups, direction)):
                result.extend(self._fields(x, y, out))
        return self.new_fieldlist_from_list(result)

    @staticmethod
    def _fields(x: Any, y: Any, out) -> Iterator[Any]:
        # the outputs keep each input's param and template (R: rotate_winds.py:86-87, :117-118)
        for template, (stack, level) in zip((x, y), out):
            yield new_field_from_stack(stack, level, template=template, metadata=dict(param=template.metadata("param")))

    def forward(self, data: Any) -> FieldList:
        return self._run(data, "forward")

    def backward(self, data: Any) -> FieldList:
        return self._run(data, "backward")

    # the per-group entry points of the reference API
    def forward_transform(self, x_wind: Any, y_wind: Any) -> Iterator[Any]:
        (out,) = self._rotate([(x_wind, y_wind)], "forward")
        yield from self._fields(x_wind, y_wind, out)

    def backward_transform(self, x_wind: Any, y_wind: Any) -> Iterator[Any]:
        (out,) = self._rotate([(x_wind, y_wind)], "backward")
        yield from self._fields(x_wind, y_wind, out)


filter_registry.register("rotate_winds", RotateWinds)
filter_registry.register("unrotate_winds", RotateWinds.reversed)
