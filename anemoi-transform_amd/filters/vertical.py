"""``ml_to_pl``: the model-level fields of a FieldList interpolated to pressure levels — an extension, the reference has no such filter.

Datasets are kept on 13 or so pressure levels; the stacks this package is tuned for hold the 137 model levels of a variable with each
point's column contiguous.  This filter is the step between the two, on the device: every ``param`` with ``levtype == "ml"`` of a group
(the fields that share every MARS key but ``param``, ``levelist`` and ``levtype``) goes through ``atx_levels_interpolate`` with the
group's surface pressure, the variables that share a level set in ONE launch as a tall stack (``vertical.interpolate_levels``).  The
results are levels of a resident stack: ``ml_to_pl | regrid`` gathers 13 levels per variable instead of 137 and never leaves HBM.

The statement (include/atx_levels.h) is in-tree: linear in pressure or in its logarithm between the two full levels that bracket the
target, the lowest level's value in the half layer above the ground, ``outside`` above the top full level and below the ground.  The
``t`` / ``z`` extrapolations of IFS below the ground are out of scope; height-level targets are ``ml_to_hl``'s (below).

``geopotential_on_model_levels`` (below) is that integral: ``z`` is not archived on IFS model levels, so it is integrated hydrostatically
from ``t``, ``q``, the surface pressure and the surface geopotential (``atx_geopotential_on_model_levels``, include/atx_geopotential.h),
and ``ml_to_pl`` takes it to pressure levels as any other variable.

``ml_to_hl`` (below) is the height-level filter on top of that integral: the model-level fields of a group at heights above the ground
or above mean sea level (wind at 10 / 100 / 200 m, ``t`` and ``q`` at the height of an observation), through ``atx_heights_interpolate``
(include/atx_heights.h) — the integral, the bracket search in it and the interpolation of every variable in ONE launch per group, without
``z`` on model levels ever being written.
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
from ..stack import Stack
from .. import native_heights
from ..vertical import geopotential_on_model_levels, interpolate_levels, interpolate_to_heights
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


class _HybridLevelFilter(Filter):
    """What the filters on hybrid model-level columns share; ``name`` is the registered name, which every message starts with."""

    def _set_table(self, name: str, model_level_AB: Any) -> None:
        self.name, (self.A, self.B) = name, _set_AB(model_level_AB)
        if self.A.shape != self.B.shape or self.A.ndim != 1 or len(self.A) < 2:
            raise ValueError(f"{self.name}: A and B must be two lists of the same length (model levels + 1), got {self.A.shape} and {self.B.shape}")
        self._device_AB: dict[Any, tuple[torch.Tensor, torch.Tensor]] = {}

    def _coefficients(self, device: Any) -> tuple[torch.Tensor, torch.Tensor]:
        if device not in self._device_AB:
            self._device_AB[device] = tuple(torch.tensor(np.asarray(c, dtype=np.float64), device=device) for c in (self.A, self.B))
        return self._device_AB[device]

    def _model_level(self, param: str, levelist: Any) -> int:
        try:
            level = int(levelist)
        except (TypeError, ValueError):
            raise ValueError(f"{self.name}: model-level field {param} has levelist {levelist!r}") from None
        if not 1 <= level <= len(self.A) - 1:
            raise ValueError(f"{self.name}: level {level} of {param} is outside the {len(self.A) - 1} model levels of the A / B table")
        return level

    def _no_surface_pressure(self, identity: Any, has_lnsp: bool) -> ValueError:
        hint = f" (it has lnsp: lnsp_to_sp | {self.name} is the route, lnsp is not taken in place of the surface pressure)" if has_lnsp else ""
        return ValueError(f"{self.name}: no surface pressure {self.surface_pressure!r} for the model-level fields of {sorted(identity)}{hint}")


@filter_registry.register("ml_to_pl")
class ModelToPressureLevels(_HybridLevelFilter):
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
        self._set_table("ml_to_pl", model_level_AB)
        self.targets_pa = [float(v) * 100.0 for v in self.levels]
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
            level = self._model_level(param, taken["levelist"])
            members = group["ml"].setdefault(param, [])
            if any(level == seen for seen, _ in members):
                raise ValueError(f"Duplicate component {param} for {identity} and level {level}")
            members.append((level, field))
        plan = []
        level_sets: dict[str, tuple[int, ...]] = {}
        for identity, group in groups.items():
            if not group["ml"]:
                continue
            if group["sp"] is None:
                raise self._no_surface_pressure(identity, group["lnsp"])
            for param, members in group["ml"].items():
                level_set = tuple(sorted(level for level, _ in members))
                if level_sets.setdefault(param, level_set) != level_set:
                    raise ValueError(f"ml_to_pl: mixed level sets for {param}: {list(level_sets[param])} and {list(level_set)} (in {sorted(identity)})")
            plan.append((group["sp"], group["ml"]))
        return passed, plan

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


GEOPOTENTIAL_PARITY_NOTE = ("geopotential_on_model_levels: the hydrostatic integral is an in-tree statement (include/atx_geopotential.h) — the IFS "
                            "discretisation as ECMWF's compute-geopotential-on-model-levels script writes it, with the moist gas constant "
                            "Rd (1 - q) + Rv q in the place of Rd Tv — and unpinned against earthkit-meteo / MARS")

#: how a COLUMNS stack is served by ``geopotential_on_model_levels``: "columns" (the LDS-tile kernel on the stacks as they are) or "fields"
#: (relayout, the FIELDS kernel, relayout back).  Set to the route that measured faster (tools/geopotential_bench.py,
#: profiles/geopotential_bench.json; DESIGN.md §3 "Geopotential kernel"): O1280 x 137 on one MI355X, "columns" 6.81 / 6.72 ms (float32 /
#: float64), "fields" with its three relayouts 7.60 / 13.16 ms — in float32 a margin of 12 % over a run-to-run spread of 1 %.  The FIELDS
#: kernel on stacks that already are field-major takes 2.70 / 4.21 ms: fields handed over in that layout stay in it.
GEOPOTENTIAL_COLUMNS_ROUTE = "columns"


@filter_registry.register("geopotential_on_model_levels")
class GeopotentialOnModelLevels(_HybridLevelFilter):
    """``z`` on model levels from ``t``, ``q``, the surface pressure and the surface geopotential — what MARS holds — so that
    ``lnsp_to_sp | geopotential_on_model_levels | ml_to_pl`` yields z500 and the rest on the device.  An extension: the reference has no
    such filter.  ``model_level_AB`` as for ``ml_to_pl``; the other arguments name the ``param`` of each input and of the output.  The
    ``t`` and ``q`` fields of a group (the fields that share every MARS key but ``param``, ``levelist`` and ``levtype``) must hold the
    same model levels, without a gap down to the lowest level of the table; the group's one ``surface_pressure`` field and its one
    ``surface_geopotential`` field (any levtype: MARS keeps it as ``z``, ``ml``, ``levelist=1``) go with them.  Every input passes
    through, except a field whose ``(param, levtype, levelist)`` an output field takes — in the default spelling the surface ``z``."""

    def __init__(self, *, model_level_AB: Any, temperature: str = "t", specific_humidity: str = "q", surface_pressure: str = "sp",
                 surface_geopotential: str = "z", output: str = "z") -> None:
        self.temperature, self.specific_humidity = temperature, specific_humidity
        self.surface_pressure, self.surface_geopotential, self.output = surface_pressure, surface_geopotential, output
        if len({temperature, specific_humidity, surface_pressure}) != 3:
            raise ValueError(f"geopotential_on_model_levels: temperature, specific_humidity and surface_pressure must be three params, got "
                             f"{temperature!r}, {specific_humidity!r}, {surface_pressure!r}")
        self._set_table("geopotential_on_model_levels", model_level_AB)
        say_once(LOG, (type(self), "parity"), GEOPOTENTIAL_PARITY_NOTE)

    def __repr__(self) -> str:
        return f"GeopotentialOnModelLevels({self.temperature!r}, {self.specific_humidity!r} -> {self.output!r})"

    # ---- grouping: host bookkeeping, every ValueError before any launch ------------------------------------------------------------
    def _plan(self, fields: list[Any]) -> tuple[list[Any], list[dict[str, Any]]]:
        """``(passed through, [group])`` in first-seen order; a group: ``sp``, ``zs``, ``levels`` (top first) and the ``t`` / ``q`` fields
        in that order."""
        name, n_model = self.name, len(self.A) - 1
        groups: dict[Any, dict[str, Any]] = {}
        owner: list[tuple[Any, Any, tuple[Any, Any, Any]]] = []  # (field, identity, (param, levtype, levelist)) in input order
        for field in fields:
            identity, taken = identity_of(field, ("param", "levelist", "levtype"), ("variable",))
            group = groups.setdefault(identity, dict(sp=None, zs=None, lnsp=False, t={}, q={}))
            param = taken["param"]
            owner.append((field, identity, (param, taken["levtype"], taken["levelist"])))
            group["lnsp"] = group["lnsp"] or param == "lnsp"
            if param == self.surface_pressure:
                if group["sp"] is not None:
                    raise ValueError(f"Duplicate component {param} for {identity}")
                group["sp"] = field
            elif param in (self.temperature, self.specific_humidity) and taken["levtype"] == "ml":
                level = self._model_level(param, taken["levelist"])
                members = group["t" if param == self.temperature else "q"]
                if level in members:
                    raise ValueError(f"Duplicate component {param} for {identity} and level {level}")
                members[level] = field
            elif param == self.surface_geopotential:  # (after t and q: a surface geopotential never shares their param on ml ... unless it is told to)
                if group["zs"] is not None:
                    raise ValueError(f"Duplicate component {param} for {identity}")
                group["zs"] = field
        plan = []
        for identity, group in groups.items():
            if not group["t"] and not group["q"]:
                continue
            for key, param in (("t", self.temperature), ("q", self.specific_humidity)):
                if not group[key]:
                    raise ValueError(f"{name}: no model-level fields of {param!r} for {sorted(identity)}")
            levels, q_levels = sorted(group["t"]), sorted(group["q"])
            if levels != q_levels:
                raise ValueError(f"{name}: mixed level sets for {self.temperature} and {self.specific_humidity}: {levels} and {q_levels} "
                                 f"(in {sorted(identity)})")
            missing = sorted(set(range(levels[0], n_model + 1)) - set(levels))
            if missing:
                raise ValueError(f"{name}: the levels {levels[0]} .. {levels[-1]} of {self.temperature} have a gap down to the lowest level "
                                 f"{n_model} of the A / B table: missing levels {missing} (in {sorted(identity)})")
            if group["sp"] is None:
                raise self._no_surface_pressure(identity, group["lnsp"])
            if group["zs"] is None:
                raise ValueError(f"{name}: no surface geopotential {self.surface_geopotential!r} for the model-level fields of {sorted(identity)}")
            plan.append(dict(identity=identity, sp=group["sp"], zs=group["zs"], levels=levels, t=[group["t"][v] for v in levels],
                             q=[group["q"][v] for v in levels]))
        taken_by_output = {(g["identity"], (self.output, "ml", level)) for g in plan for level in g["levels"]}

        def replaced(identity: Any, key: tuple[Any, Any, Any]) -> bool:
            param, levtype, levelist = key
            try:
                levelist = int(levelist)
            except (TypeError, ValueError):
                return False
            return (identity, (param, levtype, levelist)) in taken_by_output

        passed = [field for field, identity, key in owner if not replaced(identity, key)]
        return passed, plan

    def _integrate(self, group: dict[str, Any]) -> Any:
        """One stack of the group's 2 n + 2 fields (one type: float32 only if every field is), its t and q rows as two views, one launch."""
        n = len(group["levels"])
        stack = fields_to_stack([*group["t"], *group["q"], group["sp"], group["zs"]])
        relayout = stack.layout == native.COLUMNS and GEOPOTENTIAL_COLUMNS_ROUTE == "fields"
        if relayout:
            stack = stack.to_layout(native.FIELDS)
        if stack.layout == native.COLUMNS:
            rows = lambda a, b: Stack(stack.data[:, a:b], stack.n_pts, b - a, native.COLUMNS)  # noqa: E731
        else:
            rows = lambda a, b: Stack(stack.data[a:b], stack.n_pts, b - a, native.FIELDS)  # noqa: E731
        A, B = self._coefficients(stack.device)
        out = geopotential_on_model_levels(rows(0, n), rows(n, 2 * n), stack.level_view(2 * n), stack.level_view(2 * n + 1), A, B)
        return out.to_layout(native.COLUMNS) if relayout else out

    def forward(self, data: Any) -> FieldList:
        passed, plan = self._plan(list(data))
        result = list(passed)
        for group in plan:
            out = self._integrate(group)
            for k, level in enumerate(group["levels"]):
                result.append(new_field_from_stack(out, k, template=group["t"][k], metadata=dict(param=self.output, levtype="ml", levelist=level)))
        return FieldList(result)


HEIGHTS_PARITY_NOTE = ("ml_to_hl: the interpolation is an in-tree statement (include/atx_heights.h) — linear in the geopotential of the full "
                       "levels, which is the hydrostatic integral of geopotential_on_model_levels, nearest or missing outside; the heights are "
                       "geopotential heights z / g — and unpinned against earthkit-meteo, whose hybrid-to-height interpolation it resembles; "
                       "the extrapolations of IFS below the ground are not applied")


@filter_registry.register("ml_to_hl")
class ModelToHeightLevels(_HybridLevelFilter):
    """``levels``: the heights in metres (geopotential metres, ``z / g``), in the order the new fields are to come, above the ground
    (``reference="ground"``) or above mean sea level (``"sea"``; only there may a level be negative).  ``model_level_AB`` as for
    ``ml_to_pl``; ``temperature``, ``specific_humidity``, ``surface_pressure`` and ``surface_geopotential`` name the ``param`` of each
    input of the hydrostatic integral — ``lnsp`` is not taken for the surface pressure (``lnsp_to_sp | ml_to_hl``), and the surface
    geopotential is looked for under ``reference="sea"`` only: the group's ONE field of that param, of any levtype.  ``params``: only
    these are interpolated (default: every param with ml fields, ``t`` and ``q`` among them).  ``outside``: ``"nearest"`` or
    ``"missing"`` (NaN) above the top full level and below the ground.  An extension: the reference has no such filter.  The ``t``, the
    ``q`` and every interpolated param of a group (the fields that share every MARS key but ``param``, ``levelist`` and ``levtype``) must
    hold the same model levels, without a gap down to the lowest level of the table.  Every input passes through; the new fields have
    ``levtype="hl"`` and ``levelist=<metres>``."""

    def __init__(self, *, levels: Any = (10, 100, 200), model_level_AB: Any, reference: str = "ground", temperature: str = "t",
                 specific_humidity: str = "q", surface_pressure: str = "sp", surface_geopotential: str = "z", params: Any = None,
                 outside: str = "nearest") -> None:
        if isinstance(levels, (int, float)):
            levels = [levels]
        try:
            heights = [float(v) for v in levels]
        except (TypeError, ValueError):
            raise ValueError(f"ml_to_hl: levels must be heights in metres, got {levels!r}") from None
        if not heights or not all(np.isfinite(v) for v in heights):
            raise ValueError(f"ml_to_hl: levels must be a non-empty list of finite heights in metres, got {levels!r}")
        self.levels = [_level_key(v) for v in heights]
        if reference not in native_heights.REFERENCES:
            raise ValueError(f"ml_to_hl: reference must be one of {', '.join(map(repr, native_heights.REFERENCES))}, got {reference!r}")
        if reference == "ground" and any(float(v) < 0 for v in self.levels):
            raise ValueError(f"ml_to_hl: levels must not be negative above the ground (reference='sea' takes heights below sea level), got {levels!r}")
        if len(set(self.levels)) != len(self.levels):
            raise ValueError(f"ml_to_hl: duplicate levels in {levels!r}")
        if outside not in native_heights.OUTSIDE:
            raise ValueError(f"ml_to_hl: outside must be one of {', '.join(map(repr, native_heights.OUTSIDE))}, got {outside!r}")
        if len({temperature, specific_humidity, surface_pressure}) != 3:
            raise ValueError(f"ml_to_hl: temperature, specific_humidity and surface_pressure must be three params, got {temperature!r}, "
                             f"{specific_humidity!r}, {surface_pressure!r}")
        self.reference, self.outside = reference, outside
        self.temperature, self.specific_humidity = temperature, specific_humidity
        self.surface_pressure, self.surface_geopotential = surface_pressure, surface_geopotential
        self.params = None if params is None else ([params] if isinstance(params, str) else list(params))
        self._set_table("ml_to_hl", model_level_AB)
        self.heights_m = [float(v) for v in self.levels]
        say_once(LOG, (type(self), "parity"), HEIGHTS_PARITY_NOTE)

    def __repr__(self) -> str:
        return f"ModelToHeightLevels(levels={self.levels}, reference={self.reference!r}, outside={self.outside!r})"

    # ---- grouping: host bookkeeping, every ValueError before any launch ------------------------------------------------------------
    def _plan(self, fields: list[Any]) -> tuple[list[Any], list[dict[str, Any]]]:
        """``(passed through, [group])`` in first-seen order; a group: ``sp``, ``zs`` (``None`` above the ground), ``levels`` (top first),
        the ``t`` / ``q`` fields in that order, ``ml``, ``{param: fields in that order}`` of what is interpolated, and each param's template."""
        name, n_model, sea = self.name, len(self.A) - 1, self.reference == "sea"
        groups: dict[Any, dict[str, Any]] = {}
        for field in fields:
            identity, taken = identity_of(field, ("param", "levelist", "levtype"), ("variable",))
            group = groups.setdefault(identity, dict(sp=None, zs=[], lnsp=False, t={}, q={}, ml={}, templates={}))
            param, on_ml = taken["param"], taken["levtype"] == "ml"
            group["lnsp"] = group["lnsp"] or param == "lnsp"
            if param == self.surface_pressure:
                if group["sp"] is not None:
                    raise ValueError(f"Duplicate component {param} for {identity}")
                group["sp"] = field
                continue
            if param == "lnsp":  # (a model-level field in MARS, levelist 1: not a column)
                continue
            is_t_or_q = on_ml and param in (self.temperature, self.specific_humidity)
            if sea and param == self.surface_geopotential and not is_t_or_q:  # any levtype: MARS keeps it as z, ml, levelist 1
                group["zs"].append(field)
                continue
            if not on_ml:
                continue
            level = self._model_level(param, taken["levelist"])
            if is_t_or_q:
                members = group["t" if param == self.temperature else "q"]
                if level in members:
                    raise ValueError(f"Duplicate component {param} for {identity} and level {level}")
                members[level] = field
            if self.params is None or param in self.params:
                members = group["ml"].setdefault(param, {})
                if level in members:
                    raise ValueError(f"Duplicate component {param} for {identity} and level {level}")
                members[level] = field
                group["templates"].setdefault(param, field)  # the param's first ml field of the input
        plan = []
        for identity, group in groups.items():
            if not group["ml"]:
                continue
            for key, param in (("t", self.temperature), ("q", self.specific_humidity)):
                if not group[key]:
                    raise ValueError(f"{name}: no model-level fields of {param!r} for {sorted(identity)}")
            levels, q_levels = sorted(group["t"]), sorted(group["q"])
            if levels != q_levels:
                raise ValueError(f"{name}: mixed level sets for {self.temperature} and {self.specific_humidity}: {levels} and {q_levels} "
                                 f"(in {sorted(identity)})")
            for param, members in group["ml"].items():
                if sorted(members) != levels:
                    raise ValueError(f"{name}: mixed level sets for {self.temperature} and {param}: {levels} and {sorted(members)} "
                                     f"(in {sorted(identity)}; params= selects what is interpolated)")
            missing = sorted(set(range(levels[0], n_model + 1)) - set(levels))
            if missing:
                raise ValueError(f"{name}: the levels {levels[0]} .. {levels[-1]} of {self.temperature} have a gap down to the lowest level "
                                 f"{n_model} of the A / B table: missing levels {missing} (in {sorted(identity)})")
            if group["sp"] is None:
                raise self._no_surface_pressure(identity, group["lnsp"])
            if sea and not group["zs"]:
                raise ValueError(f"{name}: no surface geopotential {self.surface_geopotential!r} for the model-level fields of {sorted(identity)}")
            if sea and len(group["zs"]) > 1:
                raise ValueError(f"{name}: {len(group['zs'])} fields of the surface geopotential {self.surface_geopotential!r} for {sorted(identity)}, "
                                 f"one is needed: if geopotential_on_model_levels made them, give that filter another output= (its default "
                                 f"output takes the surface field's place), or name the surface field with surface_geopotential=")
            plan.append(dict(identity=identity, sp=group["sp"], zs=group["zs"][0] if sea else None, levels=levels,
                             t=[group["t"][v] for v in levels], q=[group["q"][v] for v in levels],
                             ml={param: [members[v] for v in levels] for param, members in group["ml"].items()}, templates=group["templates"]))
        return list(fields), plan

    def _interpolate(self, group: dict[str, Any]) -> Any:
        """One stack of the group's fields (one type: float32 only if every field is) — the variables, then t and q unless they are among
        them, then sp and zs — its rows as views, one launch."""
        n, params = len(group["levels"]), list(group["ml"])
        rows = [f for param in params for f in group["ml"][param]]
        first = {}
        for key, param in (("t", self.temperature), ("q", self.specific_humidity)):
            if param in params:
                first[key] = params.index(param) * n
            else:
                first[key] = len(rows)
                rows += group[key]
        n_rows = len(rows)
        stack = fields_to_stack([*rows, group["sp"]] + ([] if group["zs"] is None else [group["zs"]]))
        if stack.layout == native.COLUMNS:
            view = lambda a, b: Stack(stack.data[:, a:b], stack.n_pts, b - a, native.COLUMNS)  # noqa: E731
        else:
            view = lambda a, b: Stack(stack.data[a:b], stack.n_pts, b - a, native.FIELDS)  # noqa: E731
        A, B = self._coefficients(stack.device)
        zs = None if group["zs"] is None else stack.level_view(n_rows + 1)
        return interpolate_to_heights(view(0, len(params) * n), view(first["t"], first["t"] + n), view(first["q"], first["q"] + n),
                                      stack.level_view(n_rows), zs, A, B, self.heights_m, n_var=len(params), reference=self.reference,
                                      outside=self.outside)

    def forward(self, data: Any) -> FieldList:
        passed, plan = self._plan(list(data))
        result = list(passed)
        n_tgt = len(self.levels)
        for group in plan:
            out = self._interpolate(group)
            for v, param in enumerate(group["ml"]):
                template = group["templates"][param]
                for i, level in enumerate(self.levels):
                    result.append(new_field_from_stack(out, v * n_tgt + i, template=template, metadata=dict(levtype="hl", levelist=level)))
        return FieldList(result)
