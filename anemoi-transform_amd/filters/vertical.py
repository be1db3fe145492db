"""``ml_to_pl``: the model-level fields of a FieldList interpolated to pressure levels — an extension, the reference has no such filter.

Datasets are kept on 13 or so pressure levels; the stacks this package is tuned for hold the 137 model levels of a variable with each
point's column contiguous.  This filter is the step between the two, on the device: every ``param`` with ``levtype == "ml"`` of a group
(the fields that share every MARS key but ``param``, ``levelist`` and ``levtype``) goes through ``atx_levels_interpolate`` with the
group's surface pressure, the variables that share a level set in ONE launch as a tall stack (``vertical.interpolate_levels``).  The
results are levels of a resident stack: ``ml_to_pl | regrid`` gathers 13 levels per variable instead of 137 and never leaves HBM.

The statement (include/atx_levels.h) is in-tree: linear in pressure or in its logarithm between the two full levels that bracket the
target, the lowest level's value in the half layer above the ground, ``outside`` above the top full level and below the ground.  The
``t`` / ``z`` extrapolations of IFS below the ground and height-level targets (which need the geopotential integral) are out of scope.
"""

from __future__ import annotations

import logging
from typing import Any

import numpy as np
import torch

from .. import native, native_levels
from ..core import Filter, filter_registry, say_once
from ..fields import FieldList, fields_to_stack, new_field_from_stack
from ..grouping import identity_of
from ..vertical import interpolate_levels
from .domain import _one_field, _set_AB

LOG = logging.getLogger(__name__)

PARITY_NOTE = ("ml_to_pl: the interpolation is an in-tree statement (include/atx_levels.h) — linear in p or log p between full levels, "
               "nearest or missing outside — and unpinned against earthkit-meteo / MARS, whose model-to-pressure-level interpolation it "
               "resembles; the t / z extrapolations of IFS below the ground are not applied")

#: how a COLUMNS stack is served: "columns" (the LDS-tile kernel on the stack as it is) or "fields" (relayout, then the FIELDS kernel,
#: then relayout back).  Set to the route that measured faster (tools/levels_bench.py, profiles/levels_bench.json; DESIGN.md §3
#: "Level-interpolation kernel"): O1280 x 137 -> 13 levels on one MI355X, "columns" 3.80 / 4.16 ms (one float32 / float64 variable) and
#: 7.54 / 12.1 ms (five), "fields" with its two relayouts 6.62 / 8.33 and 18.3 / 27.4 ms.
COLUMNS_ROUTE = "columns"


def _level_key(level: Any) -> Any:
    """A ``levels`` entry as the ``levelist`` it becomes: whole numbers stay ints (MARS' ``levelist=850``)."""
    value = float(level)
    return int(value) if value == int(value) else value


@filter_registry.register("ml_to_pl")
class ModelToPressureLevels(Filter):
    """``levels``: the pressure levels in hPa (MARS' unit for ``levtype=pl``), in the order the new fields are to come.
    ``model_level_AB``: the half-level coefficients, a dict ``{"A": [...], "B": [...]}`` or a registered name
    (``filters.domain.register_model_level_AB``).  ``surface_pressure``: the ``param`` of the surface pressure in Pa — ``lnsp`` is not
    taken in its place (``lnsp_to_sp | ml_to_pl``).  ``params``: only these are interpolated (default: every param with ml fields).
    ``interpolation``: ``"linear"`` or ``"log"`` in pressure.  ``outside``: ``"nearest"`` or ``"missing"`` (NaN)."""

    def __init__(self, *, levels: Any, model_level_AB: Any, surface_pressure: str = "sp", params: Any = None, interpolation: str = "linear",
                 outside: str = "nearest") -> None:
        if isinstance(levels, (int, float)):
            levels = [levels]
        try:
            self.levels = [_level_key(v) for v in levels]
        except (TypeError, ValueError):
            raise ValueError(f"ml_to_pl: levels must be pressures in hPa, got {levels!r}") from None
        if not self.levels or not all(np.isfinite(float(v)) and float(v) > 0 for v in self.levels):
            raise ValueError(f"ml_to_pl: levels must be a non-empty list of positive pressures in hPa, got {levels!r}")
        if len(set(self.levels)) != len(self.levels):
            raise ValueError(f"ml_to_pl: duplicate levels in {levels!r}")
        if interpolation not in native_levels.COORDINATES:
            raise ValueError(f"ml_to_pl: interpolation must be one of {', '.join(map(repr, native_levels.COORDINATES))}, got {interpolation!r}")
        if outside not in native_levels.OUTSIDE:
            raise ValueError(f"ml_to_pl: outside must be one of {', '.join(map(repr, native_levels.OUTSIDE))}, got {outside!r}")
        self.interpolation, self.outside, self.surface_pressure = interpolation, outside, surface_pressure
        self.params = None if params is None else ([params] if isinstance(params, str) else list(params))
        self.A, self.B = _set_AB(model_level_AB)
        if self.A.shape != self.B.shape or self.A.ndim != 1 or len(self.A) < 2:
            raise ValueError(f"ml_to_pl: A and B must be two lists of the same length (model levels + 1), got {self.A.shape} and {self.B.shape}")
        self.targets_pa = [float(v) * 100.0 for v in self.levels]
        self._device_AB: dict[Any, tuple[torch.Tensor, torch.Tensor]] = {}
        say_once(LOG, (type(self), "parity"), PARITY_NOTE)

    def __repr__(self) -> str:
        return f"ModelToPressureLevels(levels={self.levels}, interpolation={self.interpolation!r}, outside={self.outside!r})"

    # ---- grouping: host bookkeeping, every ValueError before any launch ------------------------------------------------------------
    def _plan(self, fields: list[Any]) -> tuple[list[Any], list[tuple[Any, dict[str, list[tuple[int, Any]]]]]]:
        """``(passed through, [(sp field, {param: [(model level, field), ...] top first})])`` in first-seen order."""
        passed: list[Any] = []
        groups: dict[Any, dict[str, Any]] = {}
        for field in fields:
            identity, taken = identity_of(field, ("param", "levelist", "levtype"), ("variable",))
            group = groups.setdefault(identity, dict(sp=None, lnsp=False, ml={}))
            param = taken["param"]
            # (lnsp is a model-level field in MARS, levelist 1, and so is the sp that lnsp_to_sp makes of it: neither is a column)
            interpolated = (taken["levtype"] == "ml" and param not in (self.surface_pressure, "lnsp")
                            and (self.params is None or param in self.params))
            if param == self.surface_pressure:
                if group["sp"] is not None:
                    raise ValueError(f"Duplicate component {param} for {identity}")
                group["sp"] = field
            group["lnsp"] = group["lnsp"] or param == "lnsp"
            if not interpolated:
                passed.append(field)
                continue
            try:
                level = int(taken["levelist"])
            except (TypeError, ValueError):
                raise ValueError(f"ml_to_pl: model-level field {param} has levelist {taken['levelist']!r}") from None
            members = group["ml"].setdefault(param, [])
            if any(level == seen for seen, _ in members):
                raise ValueError(f"Duplicate component {param} for {identity} and level {level}")
            if not 1 <= level <= len(self.A) - 1:
                raise ValueError(f"ml_to_pl: level {level} of {param} is outside the {len(self.A) - 1} model levels of the A / B table")
            members.append((level, field))
        plan = []
        level_sets: dict[str, tuple[int, ...]] = {}
        for identity, group in groups.items():
            if not group["ml"]:
                continue
            if group["sp"] is None:
                hint = " (it has lnsp: lnsp_to_sp | ml_to_pl is the route, lnsp is not taken in place of the surface pressure)" if group["lnsp"] else ""
                raise ValueError(f"ml_to_pl: no surface pressure {self.surface_pressure!r} for the model-level fields of {sorted(identity)}{hint}")
            for param, members in group["ml"].items():
                level_set = tuple(sorted(level for level, _ in members))
                if level_sets.setdefault(param, level_set) != level_set:
                    raise ValueError(f"ml_to_pl: mixed level sets for {param}: {list(level_sets[param])} and {list(level_set)} (in {sorted(identity)})")
            plan.append((group["sp"], group["ml"]))
        return passed, plan

    def _coefficients(self, device: Any) -> tuple[torch.Tensor, torch.Tensor]:
        if device not in self._device_AB:
            self._device_AB[device] = tuple(torch.tensor(np.asarray(c, dtype=np.float64), device=device) for c in (self.A, self.B))
        return self._device_AB[device]

    def _interpolate(self, stack: Any, sp: torch.Tensor, n_var: int, levels: tuple[int, ...]) -> Any:
        A, B = self._coefficients(stack.device)
        whole = len(levels) == len(self.A) - 1  # (strictly increasing inside 1 .. H - 1: then it is 1 .. H - 1)
        index = None if whole else [level - 1 for level in levels]
        kwargs = dict(n_var=n_var, level_index=index, coordinate=self.interpolation, outside=self.outside)
        if stack.layout == native.COLUMNS and COLUMNS_ROUTE == "fields":
            return interpolate_levels(stack.to_layout(native.FIELDS), sp, A, B, self.targets_pa, **kwargs).to_layout(native.COLUMNS)
        return interpolate_levels(stack, sp, A, B, self.targets_pa, **kwargs)

    def forward(self, data: Any) -> FieldList:
        fields = list(data)
        passed, plan = self._plan(fields)
        result = list(passed)
        n_tgt = len(self.levels)
        for sp_field, by_param in plan:
            # the variables of the group that share a level set: one tall stack, one launch
            by_levels: dict[tuple[int, ...], list[str]] = {}
            templates = {param: members[0][1] for param, members in by_param.items()}  # the param's first ml field of the input
            for param, members in by_param.items():
                members.sort(key=lambda m: m[0])  # top first
                by_levels.setdefault(tuple(level for level, _ in members), []).append(param)
            outputs: dict[str, tuple[Any, int]] = {}
            for levels, params in by_levels.items():
                stack = fields_to_stack([f for param in params for _, f in by_param[param]])
                out = self._interpolate(stack, _one_field(sp_field, stack.dtype), len(params), levels)
                for v, param in enumerate(params):
                    outputs[param] = (out, v * n_tgt)
            for param in by_param:
                out, first = outputs[param]
                for t, level in enumerate(self.levels):
                    result.append(new_field_from_stack(out, first + t, template=templates[param], metadata=dict(levtype="pl", levelist=level)))
        return FieldList(result)
