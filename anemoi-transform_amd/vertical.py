"""Vertical interpolation of stacks: model levels to pressure levels (``atx_levels_interpolate``, include/atx_levels.h holds the
statement).  The layer below the ``ml_to_pl`` filter, next to ``GatherPlan`` in spirit: device stacks in, device stacks out, no host
round trip — so ``interpolate_levels`` followed by a gather reads 13 levels per variable instead of 137.
``geopotential_on_model_levels`` (``atx_geopotential_on_model_levels``, include/atx_geopotential.h) integrates ``z`` on model levels from ``t``, ``q``, the surface pressure and the
surface geopotential: the variable IFS does not archive there, and the one ``interpolate_levels`` is most often asked for.
``interpolate_to_heights`` (``atx_heights_interpolate``, include/atx_heights.h) takes the variables of a model-level stack to heights above
the ground or above the sea: that integral, the bracket search in it and the interpolation in one launch, without ``z`` in memory.
"""

from __future__ import annotations

from typing import Any, Sequence

import numpy as np
import torch

from . import native_geopotential, native_heights, native_levels
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
