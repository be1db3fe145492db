"""Vertical interpolation of stacks: model levels to pressure levels (``atx_levels_interpolate``, include/atx_levels.h holds the
statement).  The layer below the ``ml_to_pl`` filter, next to ``GatherPlan`` in spirit: device stacks in, device stacks out, no host
round trip — so ``interpolate_levels`` followed by a gather reads 13 levels per variable instead of 137.
``geopotential_on_model_levels`` (``atx_geopotential_on_model_levels``, include/atx_geopotential.h) integrates ``z`` on model levels from ``t``, ``q``, the surface pressure and the
surface geopotential: the variable IFS does not archive there, and the one ``interpolate_levels`` is most often asked for.
``interpolate_to_heights`` (``atx_heights_interpolate``, include/atx_heights.h) takes the variables of a model-level stack to heights above
the ground or above the sea: that integral, the bracket search in it and the interpolation in one launch, without ``z`` in memory.
``t_z_on_pressure_levels`` (``atx_pltz_interpolate``, include/atx_pltz.h) gives ``t`` and ``z`` on pressure levels with the IFS
extrapolations under the ground, and ``msl``: the same integral, the bracket search in pressure and both results in one launch.
``interpolate_on_coordinate`` (``atx_coord_interpolate``, include/atx_coord.h) takes the variables of ANY stack of levels to surfaces of a
second stack's values — ``z`` on pressure levels to heights, ``pt`` to isentropes: the coordinate column of every point is read, not derived.
``integrate_columns`` (``atx_integral_columns``, include/atx_integral.h) REDUCES the columns: ``1/g`` times the pressure integral of a
variable or of a product of two, or the pressure-weighted mean of a layer, on model levels or on pressure levels.
``search_columns`` (``atx_search_columns``, include/atx_search.h) SEARCHES the columns, which need not be monotone: the first step from
either end at which a search variable crosses a value — the freezing level, the dynamic tropopause, cloud base — or the level of its
maximum or minimum — the jet level — and the variables of a stack there.
``lift_parcels`` (``atx_parcel_columns``, include/atx_parcel.h) FOLLOWS a parcel through the columns of ``t`` and ``q``: CAPE, CIN and the
lifting condensation level of the lowest or of the most unstable parcel, on model levels or on pressure levels.
"""

from __future__ import annotations

from typing import Any, Sequence

import numpy as np
import torch

from . import native_coord, native_geopotential, native_heights, native_integral, native_levels, native_parcel, native_pltz, native_search
from .stack import COLUMNS, Stack

G = 9.80665  # m / s^2: metres of geopotential height to geopotential (``filters.pointwise.g_gravitational_acceleration``)


def _device_f64(values: Any, device: torch.device) -> torch.Tensor:
    if isinstance(values, torch.Tensor):
        return values.to(device=device, dtype=torch.float64).contiguous()
    return torch.tensor(np.asarray(values, dtype=np.float64).reshape(-1), dtype=torch.float64, device=device)


def _per_point(values: torch.Tensor, n_pts: int, dtype: torch.dtype, what: str) -> torch.Tensor:
    """One value per point (``sp``, ``zs``) as a contiguous vector of the stack's type."""
    values = values.reshape(-1)
    assert values.numel() == n_pts, (what, values.numel(), n_pts)
    if values.dtype != dtype or not values.is_contiguous():
        values = values.to(dtype).contiguous()
    return values


def interpolate_levels(stack: Stack, sp: torch.Tensor, A: Any, B: Any, targets_pa: Sequence[float], *, n_var: int = 1,
                       level_index: Sequence[int] | None = None, coordinate: str = "linear", outside: str = "nearest") -> Stack:
    """``stack`` holds ``n_var`` variables of ``stack.n_lev // n_var`` model levels each, variables adjacent, top level first; the result
    holds ``n_var x len(targets_pa)`` rows in the same layout and type: row ``v * n_tgt + t`` is variable ``v`` at ``targets_pa[t]`` (Pa, any
    order).  ``sp`` is the surface pressure of every point (Pa, a device tensor); ``A`` / ``B`` the half-level coefficients (host arrays
    or device tensors); ``level_index`` the rows' 0-based model levels where the stack holds a subset of the model (strictly increasing).
    ``coordinate``: ``"linear"`` or ``"log"`` in pressure; ``outside``: ``"nearest"`` or ``"missing"`` above the top full level and below
    the ground.  One launch — unless the column kernel refuses the stack because one point's ``n_var`` columns do not fit the LDS of a
    workgroup (``NotImplementedError``): then the variables are halved, down to a single one, and each part is launched into its own
    rows of the one result.  A variable's result does not depend on the others, so the bits are those of one launch."""
    if n_var < 1 or stack.n_lev % n_var:
        raise ValueError(f"a stack of {stack.n_lev} rows does not hold {n_var} variables of equally many levels")
    n_lev = stack.n_lev // n_var
    coordinate, outside = native_levels.coordinate_code(coordinate), native_levels.outside_code(outside)
    A, B = _device_f64(A, stack.device), _device_f64(B, stack.device)
    assert A.shape == B.shape, "A and B coefficients must have same shape"
    if level_index is None:  # the whole model (R: q_height.py:44-54, the same assertion)
        assert A.numel() == n_lev + 1, f"model level AB-coefficients should have one more vertical level than the stack's {n_lev}"
    targets = _device_f64(targets_pa if isinstance(targets_pa, torch.Tensor) else list(targets_pa), stack.device).reshape(-1)
    sp = _per_point(sp, stack.n_pts, stack.dtype, "sp")
    out = Stack.empty(stack.n_pts, n_var * targets.numel(), stack.dtype, stack.device, stack.layout)
    n_tgt = targets.numel()

    def launch(first: int, count: int) -> None:
        """Variables ``first .. first + count - 1``: views of the two column stacks that start at their rows and keep the pitch."""
        src, dst = (stack.data[:, first * n_lev:], out.data[:, first * n_tgt:]) if first else (stack.data, out.data)
        try:
            native_levels.interpolate(src, dst, sp, A, B, targets, n_pts=stack.n_pts, n_var=count, n_lev=n_lev, n_tgt=n_tgt, src_pitch=stack.pitch,
                                      out_pitch=out.pitch, layout=stack.layout, level_index=level_index, coordinate=coordinate, outside=outside)
        except NotImplementedError:
            if stack.layout != COLUMNS or count == 1:
                raise
            launch(first, count // 2)
            launch(first + count // 2, count - count // 2)

    launch(0, n_var)
    return out


def geopotential_on_model_levels(t: Stack, q: Stack, sp: torch.Tensor, zs: torch.Tensor | None, A: Any, B: Any) -> Stack:
    """The geopotential (m^2/s^2) on the model levels of ``t`` and ``q`` (``atx_geopotential_on_model_levels``, include/atx_geopotential.h
    holds the statement): the hydrostatic integral from the ground, which ``interpolate_levels`` then takes to pressure levels as any other
    variable.  ``t`` / ``q``: two stacks of the same shape, layout and type, top level first, holding the LOWEST ``n_lev`` levels of the
    ``A`` / ``B`` table (the whole model, or a subset such as levels 60-137 that reaches the ground).  ``sp``: the surface pressure of
    every point (Pa); ``zs``: the surface geopotential of every point, or ``None`` for 0.0 everywhere; both device tensors.  The result
    is a stack of ``n_lev`` rows in the layout and type of ``t``.  One launch."""
    if (t.n_pts, t.n_lev, t.layout) != (q.n_pts, q.n_lev, q.layout):
        raise ValueError(f"t and q differ in shape or layout: {t!r} and {q!r}")
    if t.dtype != q.dtype:
        raise ValueError(f"t and q differ in type: {t.dtype} and {q.dtype}")
    A, B = _device_f64(A, t.device), _device_f64(B, t.device)
    assert A.shape == B.shape, "A and B coefficients must have same shape"
    assert A.numel() >= t.n_lev + 1, f"model level AB-coefficients should have at least one more vertical level than the stack's {t.n_lev}"
    sp = _per_point(sp, t.n_pts, t.dtype, "sp")
    zs = None if zs is None else _per_point(zs, t.n_pts, t.dtype, "zs")
    out = Stack.empty(t.n_pts, t.n_lev, t.dtype, t.device, t.layout)
    native_geopotential.geopotential(t.data, q.data, sp, zs, A, B, out.data, n_pts=t.n_pts, n_lev=t.n_lev, t_pitch=t.pitch, q_pitch=q.pitch,
                               out_pitch=out.pitch, layout=t.layout)
    return out


def interpolate_to_heights(stack: Stack, t: Stack, q: Stack, sp: torch.Tensor, zs: torch.Tensor | None, A: Any, B: Any,
                           heights_m: Sequence[float], *, n_var: int = 1, reference: str = "ground", outside: str = "nearest") -> Stack:
    """``stack`` holds ``n_var`` variables of ``stack.n_lev // n_var`` model levels each, variables adjacent, top level first; ``t`` / ``q``
    hold the temperature and the specific humidity on the same levels: the LOWEST levels of the ``A`` / ``B`` table (the whole model, or a
    subset such as levels 60-137 that reaches the ground).  The result holds ``n_var x len(heights_m)`` rows in the layout and type of
    ``stack``: row ``v * n_tgt + i`` is variable ``v`` at ``heights_m[i]`` — geopotential metres (``z / g``, not geometric height) above
    the ground (``reference="ground"``; ``zs`` may be ``None``) or above mean sea level (``"sea"``; ``zs``, the surface geopotential of
    every point, is required), any order.  The targets the kernel sees are ``float64(h) * 9.80665``.  ``outside``: ``"nearest"`` or
    ``"missing"`` above the top full level and below the ground (``atx_heights_interpolate``, include/atx_heights.h holds the statement).
    One launch; the geopotential of the levels is never written to memory."""
    if n_var < 1 or stack.n_lev % n_var:
        raise ValueError(f"a stack of {stack.n_lev} rows does not hold {n_var} variables of equally many levels")
    n_lev = stack.n_lev // n_var
    if (t.n_pts, t.n_lev, t.layout) != (q.n_pts, q.n_lev, q.layout):
        raise ValueError(f"t and q differ in shape or layout: {t!r} and {q!r}")
    if (t.n_pts, t.n_lev, t.layout) != (stack.n_pts, n_lev, stack.layout):
        raise ValueError(f"t and q do not hold the {n_lev} levels, the points or the layout of the variables: {t!r} and {stack!r}")
    if not t.dtype == q.dtype == stack.dtype:
        raise ValueError(f"the variables, t and q differ in type: {stack.dtype}, {t.dtype} and {q.dtype}")
    reference, outside = native_heights.reference_code(reference), native_heights.outside_code(outside)
    if reference == native_heights.ABOVE_SEA and zs is None:
        raise ValueError("heights above the sea need the surface geopotential zs")
    A, B = _device_f64(A, stack.device), _device_f64(B, stack.device)
    assert A.shape == B.shape, "A and B coefficients must have same shape"
    assert A.numel() >= n_lev + 1, f"model level AB-coefficients should have at least one more vertical level than the stack's {n_lev}"
    heights = np.asarray(heights_m.cpu() if isinstance(heights_m, torch.Tensor) else list(heights_m), dtype=np.float64).reshape(-1)
    targets = _device_f64(heights * np.float64(G), stack.device)
    sp = _per_point(sp, stack.n_pts, stack.dtype, "sp")
    zs = None if zs is None or reference == native_heights.ABOVE_GROUND else _per_point(zs, stack.n_pts, stack.dtype, "zs")
    out = Stack.empty(stack.n_pts, n_var * targets.numel(), stack.dtype, stack.device, stack.layout)
    native_heights.interpolate(stack.data, out.data, t.data, q.data, sp, zs, A, B, targets, n_pts=stack.n_pts, n_var=n_var, n_lev=n_lev,
                               n_tgt=targets.numel(), src_pitch=stack.pitch, t_pitch=t.pitch, q_pitch=q.pitch, out_pitch=out.pitch,
                               layout=stack.layout, reference=reference, outside=outside)
    return out


def t_z_on_pressure_levels(t: Stack, q: Stack, sp: torch.Tensor, zs: torch.Tensor, A: Any, B: Any, targets_pa: Sequence[float], *,
                           coordinate: str = "linear", msl: bool = True) -> Stack:
    """Temperature and geopotential at ``targets_pa`` (Pa, any order) with the IFS extrapolations under the ground, and the mean sea level
    pressure (``atx_pltz_interpolate``, include/atx_pltz.h holds the statement).  ``t`` / ``q``: two stacks of the same shape, layout and
    type, top level first, holding the LOWEST ``n_lev`` levels of the ``A`` / ``B`` table (the whole model, or a subset such as levels
    60-137 that reaches the ground).  ``sp`` / ``zs``: the surface pressure (Pa) and the surface geopotential (m^2/s^2) of every point,
    device tensors.  The result holds ``2 x len(targets_pa)`` rows in the layout and type of ``t`` — ``t`` at every target, then ``z`` at
    every target — and with ``msl`` one more, the mean sea level pressure.  ``coordinate``: ``"linear"`` or ``"log"`` in pressure.  One
    launch; the geopotential of the model levels is never written to memory."""
    if (t.n_pts, t.n_lev, t.layout) != (q.n_pts, q.n_lev, q.layout):
        raise ValueError(f"t and q differ in shape or layout: {t!r} and {q!r}")
    if t.dtype != q.dtype:
        raise ValueError(f"t and q differ in type: {t.dtype} and {q.dtype}")
    coordinate = native_pltz.coordinate_code(coordinate)
    if sp is None or zs is None:
        raise ValueError("t and z on pressure levels need the surface pressure sp and the surface geopotential zs")
    A, B = _device_f64(A, t.device), _device_f64(B, t.device)
    assert A.shape == B.shape, "A and B coefficients must have same shape"
    assert A.numel() >= t.n_lev + 1, f"model level AB-coefficients should have at least one more vertical level than the stack's {t.n_lev}"
    targets = _device_f64(targets_pa if isinstance(targets_pa, torch.Tensor) else list(targets_pa), t.device).reshape(-1)
    sp, zs = _per_point(sp, t.n_pts, t.dtype, "sp"), _per_point(zs, t.n_pts, t.dtype, "zs")
    out = Stack.empty(t.n_pts, 2 * targets.numel() + (1 if msl else 0), t.dtype, t.device, t.layout)
    native_pltz.interpolate(t.data, q.data, sp, zs, out.data, A, B, targets, n_pts=t.n_pts, n_lev=t.n_lev, n_tgt=targets.numel(), t_pitch=t.pitch,
                            q_pitch=q.pitch, out_pitch=out.pitch, layout=t.layout, coordinate=coordinate, msl=msl)
    return out


def interpolate_on_coordinate(stack: Stack, coord: Stack, targets: Sequence[float], *, n_var: int = 1, offset: torch.Tensor | None = None,
                              floor: torch.Tensor | None = None, outside: str = "nearest") -> tuple[Stack, torch.Tensor]:
    """``stack`` holds ``n_var`` variables of ``stack.n_lev // n_var`` levels each, variables adjacent; ``coord`` holds the coordinate of
    every level at every point — the same levels, points, layout and type — strictly ascending or strictly descending along each point's
    column, in either direction per point.  The result holds ``n_var x len(targets)`` rows in the layout and type of ``stack``: row
    ``v * n_tgt + t`` is variable ``v`` where the coordinate equals ``targets[t]`` (float64, any order), linear in the coordinate between
    the two levels that bracket it (``atx_coord_interpolate``, include/atx_coord.h holds the statement).  ``offset``: one value per point
    added to every target ("above the ground": the surface geopotential); ``floor``: one value per point under which a target is NaN
    ("above the sea but under the ground"); both device tensors or ``None``.  ``outside``: ``"nearest"`` or ``"missing"`` beyond the
    column's two ends.  Returns ``(result, bad)``: ``bad`` is a uint8 device vector, 1 where a point's coordinate column is not strictly
    monotone (a NaN, an equal pair, a turn) and every result of the point is NaN.  One launch — unless the column kernel refuses the
    stack because one point's ``n_var`` columns do not fit the LDS of a workgroup (``NotImplementedError``): then the variables are
    halved, down to a single one, and each part is launched into its own rows of the one result, as ``interpolate_levels`` does.  A
    variable's result does not depend on the others, so the bits are those of one launch."""
    if n_var < 1 or stack.n_lev % n_var:
        raise ValueError(f"a stack of {stack.n_lev} rows does not hold {n_var} variables of equally many levels")
    n_lev = stack.n_lev // n_var
    if (coord.n_pts, coord.n_lev, coord.layout) != (stack.n_pts, n_lev, stack.layout):
        raise ValueError(f"the coordinate does not hold the {n_lev} levels, the points or the layout of the variables: {coord!r} and {stack!r}")
    if coord.dtype != stack.dtype:
        raise ValueError(f"the variables and the coordinate differ in type: {stack.dtype} and {coord.dtype}")
    outside = native_coord.outside_code(outside)
    targets = _device_f64(targets if isinstance(targets, torch.Tensor) else list(targets), stack.device).reshape(-1)
    offset = None if offset is None else _per_point(offset, stack.n_pts, stack.dtype, "offset")
    floor = None if floor is None else _per_point(floor, stack.n_pts, stack.dtype, "floor")
    n_tgt = targets.numel()
    out = Stack.empty(stack.n_pts, n_var * n_tgt, stack.dtype, stack.device, stack.layout)
    bad = torch.zeros(stack.n_pts, dtype=torch.uint8, device=stack.device)  # (zeros: no targets, no launch, nothing unusable reported)

    def launch(first: int, count: int) -> None:
        """Variables ``first .. first + count - 1``: views of the two column stacks that start at their rows and keep the pitch."""
        src, dst = (stack.data[:, first * n_lev:], out.data[:, first * n_tgt:]) if first else (stack.data, out.data)
        try:
            native_coord.interpolate(src, coord.data, dst, targets, n_pts=stack.n_pts, n_var=count, n_lev=n_lev, n_tgt=n_tgt, src_pitch=stack.pitch,
                                     coord_pitch=coord.pitch, out_pitch=out.pitch, layout=stack.layout, offset=offset, floor=floor, bad=bad,
                                     outside=outside)
        except NotImplementedError:
            if stack.layout != COLUMNS or count == 1:
                raise
            launch(first, count // 2)
            launch(first + count // 2, count - count // 2)

    launch(0, n_var)
    return out, bad


def integrate_columns(stack: Stack, sp: torch.Tensor, terms: Sequence[Any], bounds_pa: Sequence[Sequence[float]] | None, *, n_var: int, A: Any = None,
                      B: Any = None, levels_pa: Any = None, kind: str = "integral") -> Stack:
    """``stack`` holds ``n_var`` variables of ``stack.n_lev // n_var`` levels each, variables adjacent, top level first.  ``terms``: what is
    integrated — a variable's index, or a pair ``(v1, v2)`` for the product of two (``q u`` for the vapour transport).  ``bounds_pa``: the
    layers ``(top, bottom)`` in Pa, ``0 <= top < bottom``; ``None`` is the whole column, ``[(0, inf)]``.  ``A`` / ``B``: the ``n_lev + 1``
    half-level coefficients of the rows (hybrid model levels: a run of the model's table), or ``levels_pa``: the ``n_lev`` pressures of
    the rows, strictly increasing (pressure levels; levels under the ground weigh nothing and may hold NaN).  ``kind``: ``"integral"``,
    ``1/g`` times the pressure integral, or ``"mean"``, the pressure-weighted mean of the layer (NaN where the layer is empty).  The
    result holds ``len(terms) x len(bounds)`` rows in the layout and type of ``stack``: row ``t * n_bnd + b`` is term ``t`` over bound
    ``b`` (``atx_integral_columns``, include/atx_integral.h holds the statement).  One launch; a column stack whose rows, weights and block
    sums of ONE point exceed the LDS of a workgroup raises ``ValueError`` before any launch — splitting it is the caller's."""
    if n_var < 1 or stack.n_lev % n_var:
        raise ValueError(f"a stack of {stack.n_lev} rows does not hold {n_var} variables of equally many levels")
    n_lev = stack.n_lev // n_var
    kind = native_integral.kind_code(kind)
    pairs = [(int(t), -1) if isinstance(t, (int, np.integer)) else (int(t[0]), int(t[1]) if len(t) > 1 else -1) for t in terms]
    bounds = [(0.0, float("inf"))] if bounds_pa is None else [(float(top), float(bottom)) for top, bottom in bounds_pa]
    if (levels_pa is None) == (A is None or B is None):
        raise ValueError("integrate_columns: either A and B (hybrid model levels) or levels_pa (pressure levels)")
    if levels_pa is None:
        A, B = _device_f64(A, stack.device), _device_f64(B, stack.device)
        if not A.numel() == B.numel() == n_lev + 1:
            raise ValueError(f"integrate_columns: A and B must hold the {n_lev + 1} half levels of the stack's {n_lev} levels, got {A.numel()} and {B.numel()}")
    else:
        host = np.asarray(levels_pa.cpu() if isinstance(levels_pa, torch.Tensor) else levels_pa, dtype=np.float64).reshape(-1)
        if host.size != n_lev or not (np.diff(host) > 0).all() or not np.isfinite(host).all():
            raise ValueError(f"integrate_columns: levels_pa must be {n_lev} strictly increasing pressures, got {host.tolist()}")
        levels_pa = _device_f64(host, stack.device)
    sp = _per_point(sp, stack.n_pts, stack.dtype, "sp")
    out = Stack.empty(stack.n_pts, len(pairs) * len(bounds), stack.dtype, stack.device, stack.layout)
    try:
        native_integral.columns(stack.data, sp, out.data, pairs, bounds, n_pts=stack.n_pts, n_var=n_var, n_lev=n_lev, src_pitch=stack.pitch,
                                out_pitch=out.pitch, layout=stack.layout, A=A, B=B, levels_pa=levels_pa, kind=kind)
    except NotImplementedError as refused:  # (raised by the library's validation: nothing was launched)
        raise ValueError(f"integrate_columns: {refused}") from None
    return out


def search_columns(stack: Stack | None, search: Stack, targets: Sequence[float] | None, *, n_var: int = 1, direction: str = "forward",
                   mode: str = "any", level_values: Any = None, count: bool = False, spare_rows: int = 0) -> tuple[Stack | None, torch.Tensor | None]:
    """``stack`` holds ``n_var`` variables of ``stack.n_lev // n_var`` levels each, variables adjacent (``None`` with ``n_var=0``);
    ``search`` holds the search variable of every level at every point — the same levels, points, layout and type.  Nothing about a
    column is checked: it may rise, fall, turn and hold NaN.  ``direction``: ``"forward"`` reads row 0 first, ``"backward"`` the last row.
    ``mode``: ``"up"`` / ``"down"`` / ``"any"`` — the FIRST step in that order at which the search variable crosses ``targets[t]``
    (float64, any order) rising, falling or either way along the scan, every variable linear in the search variable inside the step;
    NaN where nothing crosses — or ``"max"`` / ``"min"``: the first level in that order of the column's extremum over what is not NaN,
    its values copied (one result; ``targets`` is ignored).  ``level_values``: one number per level, the same for every point (pressures,
    level numbers): one more variable, the last of the result.  The result holds ``(n_var + 1 if level_values) x n_tgt`` rows in the
    layout and type of ``search``: row ``v * n_tgt + t`` is variable ``v`` at ``targets[t]`` (``None`` where there is no such row).
    ``count=True``: also a uint8 device tensor ``[n_pts, n_tgt]``, the steps of the asked kind in the whole column (the rows equal to
    the extremum), saturating at 255 — 0: nothing crosses, above 1: the first is not the only one (``atx_search_columns``,
    include/atx_search.h holds the statement).  One launch — unless the column kernel refuses the stack because one point's ``n_var``
    columns do not fit the LDS of a workgroup (``NotImplementedError``): then the variables are halved, down to a single one, and each
    part is launched into its own rows of the one result, as ``interpolate_on_coordinate`` does.  A variable's result does not depend on
    the others, so the bits are those of one launch.  ``spare_rows``: that many more rows at the end of the result, left unwritten for the
    caller (the filters keep the count there, so that a group's new fields are levels of one stack)."""
    n_lev = search.n_lev
    if n_var < 0 or (n_var == 0) != (stack is None) or (stack is not None and stack.n_lev != n_var * n_lev):
        raise ValueError(f"search_columns: {n_var} variables of the search column's {n_lev} levels are not the stack {stack!r}")
    if stack is not None and ((stack.n_pts, stack.layout) != (search.n_pts, search.layout) or stack.dtype != search.dtype):
        raise ValueError(f"search_columns: the variables and the search column differ in points, layout or type: {stack!r} and {search!r}")
    direction, mode = native_search.direction_code(direction), native_search.mode_code(mode)
    extremum = mode in (native_search.MAX, native_search.MIN)
    if extremum:
        targets, n_tgt = None, 1
    else:
        targets = _device_f64(targets if isinstance(targets, torch.Tensor) else list(targets), search.device).reshape(-1)
        n_tgt = targets.numel()
    if level_values is not None:
        level_values = _device_f64(level_values, search.device).reshape(-1)
        if level_values.numel() != n_lev:
            raise ValueError(f"search_columns: level_values must hold the {n_lev} levels of the search column, got {level_values.numel()}")
    n_out = n_var + (level_values is not None)
    if n_out == 0 and not count:
        raise ValueError("search_columns: no variable, no level_values and no count: nothing would be written")
    n_pts, columns = search.n_pts, search.layout == COLUMNS
    out = Stack.empty(n_pts, n_out * n_tgt + spare_rows, search.dtype, search.device, search.layout) if n_out + spare_rows else None
    counted = torch.zeros(n_pts * n_tgt, dtype=torch.uint8, device=search.device) if count else None  # (zeros: no targets, no launch)

    def launch(first: int, n: int) -> None:
        """Variables ``first .. first + n - 1``: views of the two column stacks that start at their rows and keep the pitch; the part
        that holds the last variable takes level_values, whose rows follow it, and the first part the count."""
        src = None if stack is None else (stack.data[:, first * n_lev:] if first else stack.data)
        dst = None if not n_out else (out.data[:, first * n_tgt:] if first else out.data)
        try:
            native_search.columns(src, search.data, dst, targets, n_pts=n_pts, n_var=n, n_lev=n_lev, n_tgt=n_tgt, src_pitch=0 if stack is None else stack.pitch,
                                  search_pitch=search.pitch, out_pitch=0 if out is None else out.pitch, layout=search.layout, direction=direction,
                                  mode=mode, level_values=level_values if first + n == n_var else None, count=counted if first == 0 else None)
        except NotImplementedError:
            if not columns or n <= 1:
                raise
            launch(first, n // 2)
            launch(first + n // 2, n - n // 2)

    launch(0, n_var)
    if counted is not None:
        counted = counted.view(n_pts, n_tgt) if columns else counted.view(n_tgt, n_pts).t()
    return out, counted


def lift_parcels(t: Stack, q: Stack, sp: torch.Tensor, *, A: Any = None, B: Any = None, levels_pa: Any = None, parcel: str = "lowest",
                 depth_pa: float = 30000.0, top_pa: float = 5000.0, outputs: Sequence[str] = native_parcel.OUTPUTS) -> Stack:
    """``t`` and ``q`` hold the same levels of temperature (K) and specific humidity (kg / kg), top level first, in one layout and type —
    two stacks, or two views of one.  ``A`` / ``B``: the ``n_lev + 1`` half-level coefficients of the rows (hybrid model levels), or
    ``levels_pa``: the ``n_lev`` pressures of the rows, strictly increasing (pressure levels; levels under the ground take no part and may
    hold NaN).  ``parcel``: ``"lowest"``, the lowest level that takes part, or ``"most-unstable"``, the level of the largest theta_e within
    ``depth_pa`` of it; levels above ``top_pa`` take no part.  The result holds one row per name of ``outputs`` — of ``cape``, ``cin``
    (<= 0; NaN where no step holds a positive area), ``plcl``, ``tlcl``, ``pstart`` — in the layout and type of ``t``
    (``atx_parcel_columns``, include/atx_parcel.h holds the statement).  One launch; a column stack whose levels of ONE point exceed the
    LDS of a workgroup raises ``ValueError`` before any launch."""
    names = tuple(outputs)
    unknown = [name for name in names if name not in native_parcel.OUTPUTS]
    if unknown or not names:
        raise ValueError(f"lift_parcels: outputs must be some of {', '.join(native_parcel.OUTPUTS)}, got {list(outputs)}")
    if (t.n_pts, t.n_lev, t.layout, t.dtype) != (q.n_pts, q.n_lev, q.layout, q.dtype):
        raise ValueError(f"lift_parcels: t and q differ in shape, layout or type: {t} and {q}")
    n_lev = t.n_lev
    if (levels_pa is None) == (A is None or B is None):
        raise ValueError("lift_parcels: either A and B (hybrid model levels) or levels_pa (pressure levels)")
    if levels_pa is None:
        A, B = _device_f64(A, t.device), _device_f64(B, t.device)
        if not A.numel() == B.numel() == n_lev + 1:
            raise ValueError(f"lift_parcels: A and B must hold the {n_lev + 1} half levels of the stack's {n_lev} levels, got {A.numel()} and {B.numel()}")
    else:
        host = np.asarray(levels_pa.cpu() if isinstance(levels_pa, torch.Tensor) else levels_pa, dtype=np.float64).reshape(-1)
        if host.size != n_lev or not (np.diff(host) > 0).all() or not np.isfinite(host).all():
            raise ValueError(f"lift_parcels: levels_pa must be {n_lev} strictly increasing pressures, got {host.tolist()}")
        levels_pa = _device_f64(host, t.device)
    sp = _per_point(sp, t.n_pts, t.dtype, "sp")
    out = Stack.empty(t.n_pts, len(native_parcel.OUTPUTS), t.dtype, t.device, t.layout)
    try:
        native_parcel.columns(t.data, q.data, sp, out.data, n_pts=t.n_pts, n_lev=n_lev, t_pitch=t.pitch, q_pitch=q.pitch, out_pitch=out.pitch,
                              layout=t.layout, A=A, B=B, levels_pa=levels_pa, parcel=parcel, depth_pa=depth_pa, top_pa=top_pa)
    except NotImplementedError as refused:  # (raised by the library's validation: nothing was launched)
        raise ValueError(f"lift_parcels: {refused}") from None
    if names == native_parcel.OUTPUTS:
        return out
    rows = torch.tensor([native_parcel.OUTPUTS.index(name) for name in names], device=t.device)
    chosen = Stack.empty(t.n_pts, len(names), t.dtype, t.device, t.layout)
    if t.layout == COLUMNS:
        chosen.data[:, :len(names)] = out.data[:, rows]
    else:
        chosen.data[:, :t.n_pts] = out.data[rows, :t.n_pts]
    return chosen
