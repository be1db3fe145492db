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

``ml_to_pl_tz`` (below) is where ``t`` and ``z`` on pressure levels get what IFS gives them under the ground — the extrapolations that
``ml_to_pl`` leaves out — and where ``msl`` comes from: ``atx_pltz_interpolate`` (include/atx_pltz.h), the integral, the bracket search in
pressure, both variables and the mean sea level pressure in ONE launch per group.

``levels_to_coordinate`` and ``pl_to_hl`` (below) start from levels whose vertical coordinate is itself a field — pressure levels with
``z`` archived on them, any levels with ``pt`` — where the filters above derive it from the surface pressure and the A / B table:
``atx_coord_interpolate`` (include/atx_coord.h) reads the coordinate column of every point, checks that it is strictly monotone, and
interpolates every variable of the group onto its surfaces in ONE launch per group.

``vertical_integral`` (below) does not move values between levels, it REDUCES the column: total column water vapour, the integrated
vapour transport, the mass-weighted mean of a layer, on model levels or on pressure levels — ``atx_integral_columns``
(include/atx_integral.h), one launch per group.

``crossing_level`` and ``extremum_level`` (below) SEARCH the column, which need not be monotone: the freezing level where there are
inversions, the dynamic tropopause, cloud base and top, the jet level — ``atx_search_columns`` (include/atx_search.h), one launch per
group.

``parcel_ascent`` (below) FOLLOWS an air parcel through the column of ``t`` and ``q``: CAPE, CIN and the lifting condensation level of
the lowest or of the most unstable parcel, on model levels or on pressure levels — ``atx_parcel_columns`` (include/atx_parcel.h), one
launch per group.
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
from .. import native_coord, native_heights, native_integral, native_parcel, native_pltz
from ..vertical import (G, geopotential_on_model_levels, integrate_columns, interpolate_levels, interpolate_on_coordinate, interpolate_to_heights,
                        lift_parcels, search_columns, t_z_on_pressure_levels)
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


PLTZ_PARITY_NOTE = ("ml_to_pl_tz: t and z on pressure levels, their extrapolations under the ground and msl are an in-tree statement "
                    "(include/atx_pltz.h) — the ECMWF post-processing scheme as Trenberth, Berry and Buja (1993) write it, on the hydrostatic "
                    "integral of geopotential_on_model_levels — and unpinned against IFS / MARS")

#: how a COLUMNS stack is served by ``ml_to_pl_tz``: "columns" (the fused LDS-tile kernel on the stack as it is) or "fields" (relayout,
#: the FIELDS kernel, relayout back).  Set to the route that measured faster (tools/pltz_bench.py, profiles/pltz_bench.json; DESIGN.md §3
#: "Pressure-level t / z kernel"): O1280 x 137 -> 13 levels and msl on one MI355X, "columns" 8.08 / 8.87 ms (float32 / float64); the
#: FIELDS kernel on stacks that already are field-major takes 16.5 / 19.9 ms, before any relayout is counted.
PLTZ_COLUMNS_ROUTE = "columns"


@filter_registry.register("ml_to_pl_tz")
class ModelToPressureLevelsTZ(_HybridLevelFilter):
    """Temperature and geopotential on pressure levels as IFS post-processes them — interpolated between the full levels, extrapolated
    under the ground (Tibet, Greenland, Antarctica at 1000 / 925 / 850 / 700 hPa), where ``ml_to_pl`` writes the lowest level's value or
    NaN — and the mean sea level pressure, from ``t``, ``q``, the surface pressure and the surface geopotential on model levels: what
    MARS holds.  ONE launch per group (``atx_pltz_interpolate``, include/atx_pltz.h holds the statement); ``z`` on model levels is never
    written.  An extension: the reference has no such filter.

    ``levels``: the pressure levels in hPa, in the order the new fields are to come.  ``model_level_AB`` as for ``ml_to_pl``;
    ``temperature``, ``specific_humidity``, ``surface_pressure`` and ``surface_geopotential`` name the ``param`` of each input — ``lnsp``
    is not taken for the surface pressure (``lnsp_to_sp | ml_to_pl_tz``); the surface geopotential is the group's ONE field of that param,
    of any levtype (MARS keeps it as ``z``, ``ml``, ``levelist=1``).  ``interpolation``: ``"linear"`` or ``"log"`` in pressure.  The
    ``t`` and ``q`` fields of a group (the fields that share every MARS key but ``param``, ``levelist`` and ``levtype``) must hold the same
    model levels, without a gap down to the lowest level of the table.  Every input passes through; the new fields are ``temperature``
    and ``output_geopotential`` with ``levtype="pl"`` and, with ``msl=True``, ``msl`` with ``levtype="sfc"`` and no levelist.  For the
    rest of a recipe, for which the lowest level's value IS what IFS gives: ``ml_to_pl_tz | ml_to_pl(params=["u", "v", "q", "w"])``."""

    def __init__(self, *, levels: Any, model_level_AB: Any, temperature: str = "t", specific_humidity: str = "q", surface_pressure: str = "sp",
                 surface_geopotential: str = "z", interpolation: str = "linear", msl: bool = True, output_geopotential: str = "z") -> None:
        if isinstance(levels, (int, float)):
            levels = [levels]
        try:
            self.levels = [_level_key(v) for v in levels]
        except (TypeError, ValueError):
            raise ValueError(f"ml_to_pl_tz: levels must be pressures in hPa, got {levels!r}") from None
        if not self.levels or not all(np.isfinite(float(v)) and float(v) > 0 for v in self.levels):
            raise ValueError(f"ml_to_pl_tz: levels must be a non-empty list of positive pressures in hPa, got {levels!r}")
        if len(set(self.levels)) != len(self.levels):
            raise ValueError(f"ml_to_pl_tz: duplicate levels in {levels!r}")
        if interpolation not in native_pltz.COORDINATES:
            raise ValueError(f"ml_to_pl_tz: interpolation must be one of {', '.join(map(repr, native_pltz.COORDINATES))}, got {interpolation!r}")
        if len({temperature, specific_humidity, surface_pressure}) != 3:
            raise ValueError(f"ml_to_pl_tz: temperature, specific_humidity and surface_pressure must be three params, got {temperature!r}, "
                             f"{specific_humidity!r}, {surface_pressure!r}")
        self.interpolation, self.msl, self.output_geopotential = interpolation, bool(msl), output_geopotential
        self.temperature, self.specific_humidity = temperature, specific_humidity
        self.surface_pressure, self.surface_geopotential = surface_pressure, surface_geopotential
        self._set_table("ml_to_pl_tz", model_level_AB)
        self.targets_pa = [float(v) * 100.0 for v in self.levels]
        say_once(LOG, (type(self), "parity"), PLTZ_PARITY_NOTE)

    def __repr__(self) -> str:
        return f"ModelToPressureLevelsTZ(levels={self.levels}, interpolation={self.interpolation!r}, msl={self.msl})"

    # ---- grouping: host bookkeeping, every ValueError before any launch ------------------------------------------------------------
    def _plan(self, fields: list[Any]) -> tuple[list[Any], list[dict[str, Any]]]:
        """``(passed through, [group])`` in first-seen order; a group: ``sp``, ``zs``, ``levels`` (top first) and the ``t`` / ``q`` fields
        in that order."""
        name, n_model = self.name, len(self.A) - 1
        groups: dict[Any, dict[str, Any]] = {}
        for field in fields:
            identity, taken = identity_of(field, ("param", "levelist", "levtype"), ("variable",))
            group = groups.setdefault(identity, dict(sp=None, zs=[], lnsp=False, t={}, q={}))
            param = taken["param"]
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
            elif param == self.surface_geopotential:  # any levtype: MARS keeps it as z, ml, levelist 1
                group["zs"].append(field)
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
            if not group["zs"]:
                raise ValueError(f"{name}: no surface geopotential {self.surface_geopotential!r} for the model-level fields of {sorted(identity)}")
            if len(group["zs"]) > 1:
                raise ValueError(f"{name}: {len(group['zs'])} fields of the surface geopotential {self.surface_geopotential!r} for {sorted(identity)}, "
                                 f"one is needed: if geopotential_on_model_levels made them, give that filter another output= (its default "
                                 f"output takes the surface field's place), or name the surface field with surface_geopotential=")
            plan.append(dict(identity=identity, sp=group["sp"], zs=group["zs"][0], levels=levels, t=[group["t"][v] for v in levels],
                             q=[group["q"][v] for v in levels]))
        return list(fields), plan

    def _interpolate(self, group: dict[str, Any]) -> Any:
        """One stack of the group's 2 n + 2 fields (one type: float32 only if every field is), its t and q rows as two views, one launch."""
        n = len(group["levels"])
        stack = fields_to_stack([*group["t"], *group["q"], group["sp"], group["zs"]])
        relayout = stack.layout == native.COLUMNS and PLTZ_COLUMNS_ROUTE == "fields"
        if relayout:
            stack = stack.to_layout(native.FIELDS)
        if stack.layout == native.COLUMNS:
            rows = lambda a, b: Stack(stack.data[:, a:b], stack.n_pts, b - a, native.COLUMNS)  # noqa: E731
        else:
            rows = lambda a, b: Stack(stack.data[a:b], stack.n_pts, b - a, native.FIELDS)  # noqa: E731
        A, B = self._coefficients(stack.device)
        out = t_z_on_pressure_levels(rows(0, n), rows(n, 2 * n), stack.level_view(2 * n), stack.level_view(2 * n + 1), A, B, self.targets_pa,
                                     coordinate=self.interpolation, msl=self.msl)
        return out.to_layout(native.COLUMNS) if relayout else out

    def forward(self, data: Any) -> FieldList:
        passed, plan = self._plan(list(data))
        result = list(passed)
        n_tgt = len(self.levels)
        for group in plan:
            out = self._interpolate(group)
            template = group["t"][0]
            for v, param in enumerate((self.temperature, self.output_geopotential)):
                for i, level in enumerate(self.levels):
                    result.append(new_field_from_stack(out, v * n_tgt + i, template=template, metadata=dict(param=param, levtype="pl", levelist=level)))
            if self.msl:
                result.append(new_field_from_stack(out, 2 * n_tgt, template=group["sp"], metadata=dict(param="msl", levtype="sfc")))
        return FieldList(result)


COORD_PARITY_NOTE = ("levels_to_coordinate / pl_to_hl: the interpolation is an in-tree statement (include/atx_coord.h) — linear in the coordinate "
                     "field between the two levels that bracket the target, nearest or missing outside, NaN where a point's coordinate column "
                     "is not strictly monotone — and unpinned against earthkit-meteo, whose interpolation on a monotone coordinate it resembles")


@filter_registry.register("levels_to_coordinate")
class LevelsToCoordinate(Filter):
    """Every param of ``levtype`` in a group (the fields that share every MARS key but ``param``, ``levelist`` and ``levtype``) — or the
    ``params`` named — at the surfaces ``coordinate == levels[i]``, where ``coordinate`` is a param of the same group on the same levels:
    ``pt`` for isentropes, archived ``z`` for geopotential surfaces.  The coordinate of every point is read from memory
    (``atx_coord_interpolate``, include/atx_coord.h holds the statement): it may ascend or descend with ``levelist``, per point, and a
    point where it does neither gets NaN.  The group's levels are sorted by ``levelist`` before stacking, so ordinary data is monotone.
    ``outside``: ``"nearest"`` or ``"missing"`` (NaN) beyond the column's two ends.  ONE launch per group; the new fields are levels of
    one resident stack per group, float32 only if every input of the group is, with ``levtype=out_levtype`` (default: the coordinate's
    name) and ``levelist=levels[i]``.  Every input passes through.  An extension: the reference has no such filter."""

    name = "levels_to_coordinate"

    def __init__(self, *, coordinate: str = "pt", levels: Any, levtype: str = "pl", out_levtype: str | None = None, params: Any = None,
                 outside: str = "nearest") -> None:
        self._configure(coordinate, levels, levtype, coordinate if out_levtype is None else out_levtype, params, outside)
        self.targets = [float(v) for v in self.levels]

    def _configure(self, coordinate: str, levels: Any, levtype: str, out_levtype: str, params: Any, outside: str) -> None:
        name = self.name
        if isinstance(levels, (int, float)):
            levels = [levels]
        try:
            values = [float(v) for v in levels]
        except (TypeError, ValueError):
            raise ValueError(f"{name}: levels must be numbers, got {levels!r}") from None
        if not values or not all(np.isfinite(v) for v in values):
            raise ValueError(f"{name}: levels must be a non-empty list of finite numbers, got {levels!r}")
        self.levels = [_level_key(v) for v in values]
        if len(set(self.levels)) != len(self.levels):
            raise ValueError(f"{name}: duplicate levels in {levels!r}")
        if outside not in native_coord.OUTSIDE:
            raise ValueError(f"{name}: outside must be one of {', '.join(map(repr, native_coord.OUTSIDE))}, got {outside!r}")
        self.coordinate, self.levtype, self.out_levtype, self.outside = coordinate, levtype, out_levtype, outside
        self.params = None if params is None else ([params] if isinstance(params, str) else list(params))
        if self.params is not None and coordinate in self.params:
            raise ValueError(f"{name}: the coordinate {coordinate!r} is not one of the params it is interpolated on")
        self.surface, self.surface_role = None, None  # (pl_to_hl: the param of the one sfc field, and "offset" or "floor")
        say_once(LOG, (LevelsToCoordinate, "parity"), COORD_PARITY_NOTE)

    def __repr__(self) -> str:
        return f"{type(self).__name__}(coordinate={self.coordinate!r}, levels={self.levels}, levtype={self.levtype!r}, outside={self.outside!r})"

    # ---- grouping: host bookkeeping, every ValueError before any launch ------------------------------------------------------------
    def _plan(self, fields: list[Any]) -> tuple[list[Any], list[dict[str, Any]]]:
        """``(passed through, [group])`` in first-seen order; a group: ``levels`` (sorted by levelist), ``coord`` (the coordinate's fields
        in that order), ``by_param`` (``{param: fields in that order}``), each param's template and ``surface`` (a field or ``None``)."""
        name = self.name
        groups: dict[Any, dict[str, Any]] = {}
        for field in fields:
            identity, taken = identity_of(field, ("param", "levelist", "levtype"), ("variable",))
            group = groups.setdefault(identity, dict(coord={}, by_param={}, templates={}, surface=[]))
            param, levtype = taken["param"], taken["levtype"]
            if self.surface is not None and param == self.surface and levtype == "sfc":
                group["surface"].append(field)
                continue
            if levtype != self.levtype or not (param == self.coordinate or self.params is None or param in self.params):
                continue
            try:
                level = _level_key(taken["levelist"])
            except (TypeError, ValueError):
                raise ValueError(f"{name}: field {param} of levtype {levtype!r} has levelist {taken['levelist']!r}") from None
            members = group["coord"] if param == self.coordinate else group["by_param"].setdefault(param, {})
            if level in members:
                raise ValueError(f"Duplicate component {param} for {identity} and level {level}")
            members[level] = field
            if param != self.coordinate:
                group["templates"].setdefault(param, field)  # the param's first field of the input
        plan = []
        for identity, group in groups.items():
            if not group["by_param"]:
                continue
            first, levels = next((p, sorted(m, key=float)) for p, m in group["by_param"].items())
            for param, members in group["by_param"].items():
                if sorted(members, key=float) != levels:
                    raise ValueError(f"{name}: mixed level sets for {first} and {param}: {levels} and {sorted(members, key=float)} "
                                     f"(in {sorted(identity)}; params= selects what is interpolated)")
            missing = [v for v in levels if v not in group["coord"]]
            if missing:
                raise ValueError(f"{name}: the coordinate {self.coordinate!r} has no field on levels {missing} of levtype {self.levtype!r}, "
                                 f"which {first} has (in {sorted(identity)})")
            if len(group["surface"]) > 1:
                raise ValueError(f"{name}: {len(group['surface'])} sfc fields of the surface geopotential {self.surface!r} for {sorted(identity)}, "
                                 f"one is needed")
            if self.surface_role == "offset" and not group["surface"]:
                raise ValueError(f"{name}: no sfc field of the surface geopotential {self.surface!r} for {sorted(identity)}: heights above the "
                                 f"ground need it (reference='sea' does not)")
            plan.append(dict(identity=identity, levels=levels, coord=[group["coord"][v] for v in levels], templates=group["templates"],
                             by_param={param: [members[v] for v in levels] for param, members in group["by_param"].items()},
                             surface=group["surface"][0] if group["surface"] else None))
        return list(fields), plan

    def _interpolate(self, group: dict[str, Any]) -> tuple[Any, torch.Tensor]:
        """One stack of the group's fields (one type: float32 only if every field is) — the variables, the coordinate, the surface field —
        its rows as views, one launch."""
        n, params = len(group["levels"]), list(group["by_param"])
        rows = [f for param in params for f in group["by_param"][param]] + group["coord"]
        stack = fields_to_stack(rows + ([] if group["surface"] is None else [group["surface"]]))
        if stack.layout == native.COLUMNS:
            view = lambda a, b: Stack(stack.data[:, a:b], stack.n_pts, b - a, native.COLUMNS)  # noqa: E731
        else:
            view = lambda a, b: Stack(stack.data[a:b], stack.n_pts, b - a, native.FIELDS)  # noqa: E731
        surface = None if group["surface"] is None else stack.level_view(len(rows))
        return interpolate_on_coordinate(view(0, len(params) * n), view(len(params) * n, len(rows)), self.targets, n_var=len(params),
                                         offset=surface if self.surface_role == "offset" else None,
                                         floor=surface if self.surface_role == "floor" else None, outside=self.outside)

    def forward(self, data: Any) -> FieldList:
        passed, plan = self._plan(list(data))
        result = list(passed)
        n_tgt = len(self.levels)
        unusable = None
        for group in plan:
            out, bad = self._interpolate(group)
            count = bad.sum(dtype=torch.int64)
            unusable = count if unusable is None else unusable + count
            for v, param in enumerate(group["by_param"]):
                template = group["templates"][param]
                for i, level in enumerate(self.levels):
                    result.append(new_field_from_stack(out, v * n_tgt + i, template=template, metadata=dict(levtype=self.out_levtype, levelist=level)))
        if unusable is not None and int(unusable) > 0:  # (one read of one number per call, after every launch is queued)
            LOG.warning("%s: the coordinate %r is not strictly monotone at %d points of %d groups: every result there is NaN", self.name,
                        self.coordinate, int(unusable), len(plan))
        return FieldList(result)


@filter_registry.register("pl_to_hl")
class PressureToHeightLevels(LevelsToCoordinate):
    """``levels_to_coordinate`` spelled for heights: every param of ``levtype`` in a group at ``levels`` metres (geopotential metres,
    ``z / g``; the targets the kernel sees are ``float64(h) * 9.80665``), from the ``geopotential`` param on the same levels — what ERA5
    and every dataset on pressure levels archive, so hub-height wind is ``pl_to_hl(levels=[100], params=["u", "v"])``.
    ``reference="ground"``: above the ground — the group's ONE ``sfc`` field of ``surface_geopotential`` is added to every target of a
    point.  ``reference="sea"``: above mean sea level; where that field is present a height under the ground is NaN, and only under
    this reference may a level be negative.  ``levtype="ml"`` works the same way on geopotential that is on model levels:
    ``geopotential_on_model_levels | pl_to_hl(levtype="ml")``.  The new fields have ``levtype="hl"`` and ``levelist=<metres>``; the rest
    is ``levels_to_coordinate``'s."""

    name = "pl_to_hl"

    def __init__(self, *, levels: Any = (10, 100, 200), reference: str = "ground", geopotential: str = "z", surface_geopotential: str = "z",
                 levtype: str = "pl", params: Any = None, outside: str = "nearest") -> None:
        if reference not in ("ground", "sea"):
            raise ValueError(f"pl_to_hl: reference must be one of 'ground', 'sea', got {reference!r}")
        self._configure(geopotential, list(levels) if isinstance(levels, tuple) else levels, levtype, "hl", params, outside)
        if reference == "ground" and any(float(v) < 0 for v in self.levels):
            raise ValueError(f"pl_to_hl: levels must not be negative above the ground (reference='sea' takes heights below sea level), got {levels!r}")
        self.reference, self.geopotential = reference, geopotential
        self.surface, self.surface_role = surface_geopotential, "offset" if reference == "ground" else "floor"
        self.targets = list(np.array([float(v) for v in self.levels], dtype=np.float64) * np.float64(G))


INTEGRAL_PARITY_NOTE = ("vertical_integral: the column integral is an in-tree statement (include/atx_integral.h) — on model levels the finite-volume "
                        "sum over the layers between half levels, on pressure levels the trapezoid between the levels above the ground and "
                        "the lowest of them held down to the surface pressure, summed in blocks of 8 levels — and unpinned against "
                        "earthkit-meteo / IFS")

#: how a COLUMNS stack is served by ``vertical_integral``, per levtype: "columns" (the LDS-tile kernel on the stack as it is) or "fields"
#: (relayout, then the FIELDS kernel, then relayout back).  Set to the route that measured faster (tools/integral_bench.py,
#: profiles/integral_bench.json; DESIGN.md §3 "Column-integral kernel"), float32 / float64 on one MI355X: O1280 x 137 model levels, three
#: outputs, "columns" 6.44 / 9.26 ms against 10.3 / 15.3 ms with the two relayouts; 0.25 degrees x 13 pressure levels, three outputs and
#: a layer mean, "columns" 0.427 / 0.520 ms against 0.332 / 0.406 ms; run-to-run 8.6 / 5.8 %.
INTEGRAL_COLUMNS_ROUTE = {"ml": "columns", "pl": "fields"}


@filter_registry.register("vertical_integral")
class VerticalIntegral(_HybridLevelFilter):
    """Column integrals and layer means of a group (the fields that share every MARS key but ``param``, ``levelist`` and ``levtype``):
    ``outputs={"tcwv": "q", "viwve": ["q", "u"], "viwvn": ["q", "v"]}`` names each new field and the param — or the two params whose
    product — it integrates: ``1/g`` times the pressure integral (``kind="integral"``) or the pressure-weighted mean (``kind="mean"``),
    over the whole column or over each of ``layers=[[850, 500], …]`` (hPa, either order).  ``levtype="ml"``: hybrid model levels with
    ``model_level_AB`` as for ``ml_to_pl`` — the levels of a group must be one run of the table without a gap, which need not reach the
    ground; ``levtype="pl"``: pressure levels, no table — levels under the ground weigh nothing, whatever they hold.  Every param of
    ``outputs`` must hold the same levels, and the group exactly one ``surface_pressure`` field (Pa; ``lnsp`` is not taken in its place:
    ``lnsp_to_sp | vertical_integral``).  ONE launch per group (``atx_integral_columns``, include/atx_integral.h holds the statement); the
    new fields — ``param=<output name>``, with ``layers`` ``<name>_<top>_<bottom>`` in hPa as given, ``levtype="sfc"`` — are levels of one
    resident stack per group, float32 only if every input is.  Every input passes through.  An extension: the reference has no such
    filter."""

    def __init__(self, *, outputs: Any, levtype: str = "ml", model_level_AB: Any = None, surface_pressure: str = "sp", layers: Any = None,
                 kind: str = "integral") -> None:
        self.name = "vertical_integral"
        if levtype not in ("ml", "pl"):
            raise ValueError(f"vertical_integral: levtype must be 'ml' or 'pl', got {levtype!r}")
        if (levtype == "ml") != (model_level_AB is not None):
            raise ValueError("vertical_integral: levtype='ml' needs model_level_AB, levtype='pl' takes no table")
        if kind not in native_integral.KINDS:
            raise ValueError(f"vertical_integral: kind must be one of {', '.join(map(repr, native_integral.KINDS))}, got {kind!r}")
        if not isinstance(outputs, dict) or not outputs:
            raise ValueError(f"vertical_integral: outputs must be a non-empty dict of name -> param or [param, param], got {outputs!r}")
        self.outputs: dict[str, tuple[str, ...]] = {}
        for name, factors in outputs.items():
            factors = (factors,) if isinstance(factors, str) else tuple(factors)
            if len(factors) not in (1, 2) or not all(isinstance(p, str) for p in factors):
                raise ValueError(f"vertical_integral: output {name!r} must name one param or two, got {outputs[name]!r}")
            self.outputs[str(name)] = factors
        self.params = list(dict.fromkeys(p for factors in self.outputs.values() for p in factors))  # first named first
        if surface_pressure in self.params:
            raise ValueError(f"vertical_integral: the surface pressure {surface_pressure!r} is not one of the params it weighs")
        self.terms = [(self.params.index(f[0]), self.params.index(f[1]) if len(f) == 2 else -1) for f in self.outputs.values()]
        self.layers, self.bounds_pa = None, None
        if layers is not None:
            try:
                self.layers = [(_level_key(a), _level_key(b)) for a, b in layers]
            except (TypeError, ValueError):
                raise ValueError(f"vertical_integral: layers must be pairs of pressures in hPa, got {layers!r}") from None
            if not self.layers or not all(np.isfinite(float(v)) and float(v) >= 0 for pair in self.layers for v in pair) or any(a == b for a, b in self.layers):
                raise ValueError(f"vertical_integral: layers must be a non-empty list of pairs of two different pressures in hPa, got {layers!r}")
            self.bounds_pa = [(min(float(a), float(b)) * 100.0, max(float(a), float(b)) * 100.0) for a, b in self.layers]
        self.levtype, self.kind, self.surface_pressure = levtype, kind, surface_pressure
        if levtype == "ml":
            self._set_table(self.name, model_level_AB)
        say_once(LOG, (type(self), "parity"), INTEGRAL_PARITY_NOTE)

    def __repr__(self) -> str:
        return f"VerticalIntegral(outputs={self.outputs}, levtype={self.levtype!r}, layers={self.layers}, kind={self.kind!r})"

    def output_names(self) -> list[str]:
        """The params of the new fields in the order of the result's rows: output by output, layer by layer."""
        if self.layers is None:
            return list(self.outputs)
        return [f"{name}_{a}_{b}" for name in self.outputs for a, b in self.layers]

    # ---- grouping: host bookkeeping, every ValueError before any launch ------------------------------------------------------------
    def _plan(self, fields: list[Any]) -> tuple[list[Any], list[dict[str, Any]]]:
        """``(passed through, [group])`` in first-seen order; a group: ``sp``, ``levels`` (top first) and ``by_param``, the fields of every
        param of ``outputs`` in that order."""
        name = self.name
        groups: dict[Any, dict[str, Any]] = {}
        for field in fields:
            identity, taken = identity_of(field, ("param", "levelist", "levtype"), ("variable",))
            group = groups.setdefault(identity, dict(sp=[], lnsp=False, by_param={}))
            param = taken["param"]
            group["lnsp"] = group["lnsp"] or param == "lnsp"
            if param == self.surface_pressure:
                group["sp"].append(field)
            elif param in self.params and taken["levtype"] == self.levtype:
                if self.levtype == "ml":
                    level = self._model_level(param, taken["levelist"])
                else:
                    try:
                        level = _level_key(taken["levelist"])
                    except (TypeError, ValueError):
                        raise ValueError(f"{name}: pressure-level field {param} has levelist {taken['levelist']!r}") from None
                members = group["by_param"].setdefault(param, {})
                if level in members:
                    raise ValueError(f"Duplicate component {param} for {identity} and level {level}")
                members[level] = field
        plan = []
        for identity, group in groups.items():
            if not group["by_param"]:
                continue
            first = next(iter(group["by_param"]))
            levels = sorted(group["by_param"][first], key=float)
            for param in self.params:
                held = sorted(group["by_param"].get(param, {}), key=float)
                if held != levels:
                    raise ValueError(f"{name}: mixed level sets for {first} and {param}: {levels} and {held} (in {sorted(identity)})")
            if self.levtype == "ml":
                missing = sorted(set(range(levels[0], levels[-1] + 1)) - set(levels))
                if missing:
                    raise ValueError(f"{name}: the levels {levels[0]} .. {levels[-1]} of {first} are not one run of the A / B table: missing "
                                     f"levels {missing} (in {sorted(identity)})")
            if not group["sp"]:
                raise self._no_surface_pressure(identity, group["lnsp"])
            if len(group["sp"]) > 1:
                raise ValueError(f"Duplicate component {self.surface_pressure} for {identity}")
            plan.append(dict(identity=identity, sp=group["sp"][0], levels=levels,
                             by_param={param: [group["by_param"][param][v] for v in levels] for param in self.params}))
        return list(fields), plan

    def _integrate(self, group: dict[str, Any]) -> Any:
        """One stack of the group's fields (one type: float32 only if every field is) — the variables, then sp — one launch."""
        levels, n = group["levels"], len(group["levels"])
        rows = [f for param in self.params for f in group["by_param"][param]]
        stack = fields_to_stack([*rows, group["sp"]])
        relayout = stack.layout == native.COLUMNS and INTEGRAL_COLUMNS_ROUTE[self.levtype] == "fields"
        if relayout:
            stack = stack.to_layout(native.FIELDS)
        data = stack.data[:, :len(rows)] if stack.layout == native.COLUMNS else stack.data[:len(rows)]
        variables = Stack(data, stack.n_pts, len(rows), stack.layout)
        if self.levtype == "ml":
            A, B = (c[levels[0] - 1:levels[-1] + 1] for c in self._coefficients(stack.device))
            table = dict(A=A, B=B)
        else:
            table = dict(levels_pa=[float(v) * 100.0 for v in levels])
        out = integrate_columns(variables, stack.level_view(len(rows)), self.terms, self.bounds_pa, n_var=len(self.params), kind=self.kind, **table)
        return out.to_layout(native.COLUMNS) if relayout else out

    def forward(self, data: Any) -> FieldList:
        passed, plan = self._plan(list(data))
        result = list(passed)
        names = self.output_names()
        for group in plan:
            out = self._integrate(group)
            for row, name in enumerate(names):
                result.append(new_field_from_stack(out, row, template=group["sp"], metadata=dict(param=name, levtype="sfc")))
        return FieldList(result)


SEARCH_PARITY_NOTE = ("crossing_level / extremum_level: the search is an in-tree statement (include/atx_search.h) — the first step from the ground "
                      "or from the top at which the search param crosses the value, linear inside the step; the first level of the extremum — "
                      "and unpinned against earthkit-meteo and IFS, whose freezing level (deg0l) has further rules for a second warm layer")

#: how a COLUMNS stack is served by ``crossing_level`` / ``extremum_level``, per levtype: "columns" (the LDS-tile kernel with the
#: wave-cooperative search on the stack as it is) or "fields" (relayout, then the FIELDS kernel, then relayout back).  Set to the route
#: that measured faster (tools/search_bench.py, profiles/search_bench.json; DESIGN.md §3 "Column-search kernel"), float32 / float64 on
#: one MI355X, z, u, v out: O1280 x 137 model levels, the 273.15 K crossing "columns" 4.68 / 7.59 ms against 7.58 / 13.5 ms with the
#: relayouts, the maximum 5.23 / 8.12 against 8.44 / 14.3 ms; 0.25 degrees x 13 pressure levels, 0.293 / 0.349 against 0.265 / 0.327 ms
#: and 0.282 / 0.329 against 0.254 / 0.351 ms — differences of 10 % under a run-to-run spread of 13 - 19 %: no route is shown faster
#: there, and the stack stays as it is.  Height levels were not measured.
SEARCH_COLUMNS_ROUTE = {"ml": "columns", "pl": "columns", "hl": "columns"}

LEVELIST = "levelist"  # the reserved source of an output: the levelist at the answer, interpolated as a variable is


class _ColumnSearch(Filter):
    """What ``crossing_level`` and ``extremum_level`` share: a group is the fields that share every MARS key but ``param``, ``levelist``
    and ``levtype``; its ``search`` param and every source of ``outputs`` on ``levtype`` must hold the same levels, which are sorted by
    ``levelist`` before stacking.  ``start``: the end of the column the scan starts from — the ground is the largest ``levelist`` on
    ``pl`` and ``ml``, the smallest on ``hl``.  ONE launch per group; the new fields (``levtype="sfc"``) are levels of one resident stack
    per group, float32 only if every input is.  Every input passes through."""

    name = "column_search"

    def _configure(self, search: str, outputs: Any, levtype: str, start: str, count: Any) -> None:
        name = self.name
        if levtype not in SEARCH_COLUMNS_ROUTE:
            raise ValueError(f"{name}: levtype must be one of {', '.join(map(repr, SEARCH_COLUMNS_ROUTE))}, got {levtype!r}")
        if start not in ("ground", "top"):
            raise ValueError(f"{name}: start must be one of 'ground', 'top', got {start!r}")
        if not isinstance(outputs, dict) or not all(isinstance(k, str) and isinstance(v, str) for k, v in outputs.items()):
            raise ValueError(f"{name}: outputs must be a dict of name -> param (or 'levelist'), got {outputs!r}")
        if count is not None and not isinstance(count, str):
            raise ValueError(f"{name}: count must name the new field, got {count!r}")
        if not outputs and count is None:
            raise ValueError(f"{name}: no outputs and no count: nothing would be written")
        if count is not None and count in outputs:
            raise ValueError(f"{name}: the count {count!r} is also one of the outputs")
        self.search, self.outputs, self.levtype, self.start, self.count = search, dict(outputs), levtype, start, count
        self.variables = [source for source in self.outputs.values() if source != LEVELIST]  # one per output that is not the levelist
        self.with_levelist = LEVELIST in self.outputs.values()
        # ground last on pl / ml (the rows are sorted by levelist), first on hl
        ground_first = levtype == "hl"
        self.direction = "forward" if (start == "ground") == ground_first else "backward"
        self.values: list[Any] = []
        say_once(LOG, (_ColumnSearch, "parity"), SEARCH_PARITY_NOTE)

    def output_names(self) -> list[str]:
        """The params of the new fields in their order: output by output, value by value, then the count's."""
        names = list(self.outputs) + ([] if self.count is None else [self.count])
        if len(self.values) <= 1:
            return names
        return [f"{name}_{value}" for name in names for value in self.values]

    # ---- grouping: host bookkeeping, every ValueError before any launch ------------------------------------------------------------
    def _plan(self, fields: list[Any]) -> tuple[list[Any], list[dict[str, Any]]]:
        """``(passed through, [group])`` in first-seen order; a group: ``levels`` (sorted by levelist) and ``by_param``, the fields of
        the search param and of every source in that order."""
        name, wanted = self.name, {self.search, *self.variables}
        groups: dict[Any, dict[str, dict[Any, Any]]] = {}
        for field in fields:
            identity, taken = identity_of(field, ("param", "levelist", "levtype"), ("variable",))
            group = groups.setdefault(identity, {})
            if taken["levtype"] != self.levtype or taken["param"] not in wanted:
                continue
            try:
                level = _level_key(taken["levelist"])
            except (TypeError, ValueError):
                raise ValueError(f"{name}: field {taken['param']} of levtype {self.levtype!r} has levelist {taken['levelist']!r}") from None
            members = group.setdefault(taken["param"], {})
            if level in members:
                raise ValueError(f"Duplicate component {taken['param']} for {identity} and level {level}")
            members[level] = field
        plan = []
        for identity, group in groups.items():
            if not group:
                continue
            if self.search not in group:
                raise ValueError(f"{name}: no fields of the search param {self.search!r} on levtype {self.levtype!r} for {sorted(identity)}")
            levels = sorted(group[self.search], key=float)
            for param in self.variables:
                if param not in group:
                    raise ValueError(f"{name}: no fields of the output param {param!r} on levtype {self.levtype!r} for {sorted(identity)}")
                if sorted(group[param], key=float) != levels:
                    raise ValueError(f"{name}: mixed level sets for {self.search} and {param}: {levels} and {sorted(group[param], key=float)} "
                                     f"(in {sorted(identity)})")
            plan.append(dict(identity=identity, levels=levels, by_param={param: [members[v] for v in levels] for param, members in group.items()}))
        return list(fields), plan

    def _search(self, group: dict[str, Any]) -> tuple[Any, int]:
        """One stack of the group's fields (one type: float32 only if every field is) — a variable per output, then the search column —
        its rows as views, one launch; the count, where asked, goes into the spare rows of the result.  Returns the result and the rows
        of the kernel's own outputs."""
        n, n_var = len(group["levels"]), len(self.variables)
        stack = fields_to_stack([f for param in self.variables for f in group["by_param"][param]] + group["by_param"][self.search])
        relayout = stack.layout == native.COLUMNS and SEARCH_COLUMNS_ROUTE[self.levtype] == "fields"
        if relayout:
            stack = stack.to_layout(native.FIELDS)
        if stack.layout == native.COLUMNS:
            view = lambda a, b: Stack(stack.data[:, a:b], stack.n_pts, b - a, native.COLUMNS)  # noqa: E731
        else:
            view = lambda a, b: Stack(stack.data[a:b], stack.n_pts, b - a, native.FIELDS)  # noqa: E731
        n_tgt = max(1, len(self.values))
        out, counted = search_columns(view(0, n_var * n) if n_var else None, view(n_var * n, (n_var + 1) * n), self.values, n_var=n_var,
                                      direction=self.direction, mode=self.mode, count=self.count is not None,
                                      level_values=[float(v) for v in group["levels"]] if self.with_levelist else None,
                                      spare_rows=n_tgt if self.count is not None else 0)
        rows = (n_var + self.with_levelist) * n_tgt
        if counted is not None:
            for t in range(n_tgt):
                out.level_view(rows + t).copy_(counted[:, t])
        return (out.to_layout(native.COLUMNS) if relayout else out), rows

    def forward(self, data: Any) -> FieldList:
        passed, plan = self._plan(list(data))
        result = list(passed)
        n_tgt = max(1, len(self.values))
        variable_row = {}
        for name, source in self.outputs.items():  # the kernel's rows: the variables in the order of outputs, the levelist last
            variable_row[name] = len(self.variables) if source == LEVELIST else len([k for k in variable_row if self.outputs[k] != LEVELIST])
        names = self.output_names()
        for group in plan:
            out, rows = self._search(group)
            first = [variable_row[name] * n_tgt for name in self.outputs] + ([] if self.count is None else [rows])
            for i, name in enumerate(names):
                source = ([*self.outputs.values()] + [LEVELIST])[i // n_tgt]
                template = group["by_param"][self.search if source == LEVELIST else source][0]
                result.append(new_field_from_stack(out, first[i // n_tgt] + i % n_tgt, template=template,
                                                   metadata=dict(param=name, levtype="sfc", levelist=None)))
        return FieldList(result)


@filter_registry.register("crossing_level")
class CrossingLevel(_ColumnSearch):
    """The first level, from the ground or from the top, at which ``search`` crosses each of ``values``, and what ``outputs`` name there:
    ``crossing_level(search="t", values=[273.15], outputs={"deg0l": "z"})`` is the height of the freezing level where the column has
    inversions, which ``levels_to_coordinate`` refuses; ``search="pv", values=[2e-6], start="top", outputs={"ptrop": "levelist"}`` the
    dynamic tropopause; a ``cc`` threshold from either end cloud base and cloud top.  ``sense``: ``"rising"`` / ``"falling"`` ALONG THE
    SCAN (from ``start``), or ``"any"``.  An output's source is a param of the group on the same levels, or ``"levelist"``; every output
    is linear in ``search`` inside the step that crosses, NaN where no step does.  With several ``values`` the new fields are
    ``<name>_<value>``.  ``count="name"``: one more field, the number of crossings of the asked sense in the whole column (255 at most).
    An extension: the reference has no such filter."""

    name = "crossing_level"
    SENSES = {"any": "any", "rising": "up", "falling": "down"}

    def __init__(self, *, search: str = "t", values: Any = (273.15,), start: str = "ground", sense: str = "any", outputs: Any = None,
                 levtype: str = "pl", count: Any = None) -> None:
        if sense not in self.SENSES:
            raise ValueError(f"{self.name}: sense must be one of {', '.join(map(repr, self.SENSES))}, got {sense!r}")
        self._configure(search, {} if outputs is None else outputs, levtype, start, count)
        if isinstance(values, (int, float)):
            values = [values]
        try:
            numbers = [float(v) for v in values]
        except (TypeError, ValueError):
            raise ValueError(f"{self.name}: values must be numbers, got {values!r}") from None
        if not numbers or not all(np.isfinite(v) for v in numbers):
            raise ValueError(f"{self.name}: values must be a non-empty list of finite numbers, got {values!r}")
        self.values = [_level_key(v) for v in numbers]
        if len(set(self.values)) != len(self.values):
            raise ValueError(f"{self.name}: duplicate values in {values!r}")
        self.sense, self.mode = sense, self.SENSES[sense]

    def __repr__(self) -> str:
        return f"CrossingLevel(search={self.search!r}, values={self.values}, start={self.start!r}, sense={self.sense!r}, levtype={self.levtype!r})"


@filter_registry.register("extremum_level")
class ExtremumLevel(_ColumnSearch):
    """The level of the maximum (``kind="maximum"``) or minimum of ``search`` over a column, the first from ``start`` among equals, NaN
    levels apart, and what ``outputs`` name there, copied: ``extremum_level(search="ws", outputs={"zjet": "z", "ujet": "u"})`` is the
    jet level.  An output's source is a param of the group on the same levels, or ``"levelist"``.  ``count="name"``: one more field, the
    number of levels equal to the extremum.  It takes no ``values``.  An extension: the reference has no such filter."""

    name = "extremum_level"
    KINDS = {"maximum": "max", "minimum": "min"}

    def __init__(self, *, search: str = "ws", kind: str = "maximum", start: str = "ground", outputs: Any = None, levtype: str = "pl",
                 count: Any = None, values: Any = None) -> None:
        if values is not None:
            raise ValueError(f"{self.name}: an extremum takes no values, got {values!r} (crossing_level does)")
        if kind not in self.KINDS:
            raise ValueError(f"{self.name}: kind must be one of {', '.join(map(repr, self.KINDS))}, got {kind!r}")
        self._configure(search, {} if outputs is None else outputs, levtype, start, count)
        self.kind, self.mode = kind, self.KINDS[kind]

    def __repr__(self) -> str:
        return f"ExtremumLevel(search={self.search!r}, kind={self.kind!r}, start={self.start!r}, levtype={self.levtype!r})"


PARCEL_PARITY_NOTE = ("parcel_ascent: the ascent is an in-tree statement (include/atx_parcel.h) — Bolton's T_L and theta_e, the pseudo-adiabat of "
                      "constant theta_e solved per level, trapezoids of the virtual-temperature buoyancy in ln p split at its zeros — and unpinned "
                      "against earthkit-meteo, metpy and IFS, whose cape follows parcel rules of its own")

#: how a COLUMNS stack is served by ``parcel_ascent``, per levtype: "columns" (the LDS-tile kernel with a lane per (point, level) on the
#: stack as it is) or "fields" (relayout, then the FIELDS kernel, then relayout back).  Set to the route that measured faster
#: (tools/parcel_bench.py, profiles/parcel_bench.json; DESIGN.md §3 "Parcel kernel"), float32 / float64 on one MI355X, the lowest parcel:
#: O1280 x 137 model levels "columns" 97.0 / 92.8 ms against 57.0 / 60.2 ms with the relayouts; 0.25 degrees x 13 pressure levels 1.99 /
#: 2.00 against 1.60 / 1.62 ms — differences of 20 - 41 % over a run-to-run spread of 0.1 - 2.4 %.  In the field-major kernel the 64 lanes
#: of a wave stand at ONE level, so a level below the LCL skips its Newton steps for the whole wave; in the column kernel a wave holds
#: levels of both kinds and runs them for all.  The most unstable parcel was not measured.
PARCEL_COLUMNS_ROUTE = {"ml": "fields", "pl": "fields"}


@filter_registry.register("parcel_ascent")
class ParcelAscent(_HybridLevelFilter):
    """CAPE, CIN and the lifting condensation level of a group (the fields that share every MARS key but ``param``, ``levelist`` and
    ``levtype``): ``outputs={"cape": "cape", "cin": "cin", "plcl": "plcl"}`` names, for each of ``cape``, ``cin`` (J / kg, <= 0, NaN where
    the parcel is nowhere buoyant), ``plcl`` (Pa), ``tlcl`` (K) and ``pstart`` (Pa) that is wanted, the param of the new field.
    ``parcel="lowest"``: the parcel of the lowest level above the ground; ``"most-unstable"``: of the level of the largest theta_e in the
    lowest ``depth`` hPa.  Levels above ``top`` hPa take no part.  ``levtype="ml"``: hybrid model levels with ``model_level_AB`` as for
    ``ml_to_pl`` — the levels of a group must be one run of the table without a gap; ``levtype="pl"``: pressure levels, no table — levels
    under the ground take no part, whatever they hold.  ``temperature`` and ``specific_humidity`` must hold the same levels, and the
    group exactly one ``surface_pressure`` field (Pa; ``lnsp`` is not taken in its place: ``lnsp_to_sp | parcel_ascent``).  ONE launch per
    group (``atx_parcel_columns``, include/atx_parcel.h holds the statement); the new fields, ``levtype="sfc"``, are levels of one resident
    stack per group, float32 only if every input is.  Every input passes through.  An extension: the reference has no such filter."""

    def __init__(self, *, outputs: Any = None, levtype: str = "pl", model_level_AB: Any = None, temperature: str = "t", specific_humidity: str = "q",
                 surface_pressure: str = "sp", parcel: str = "lowest", depth: float = 300, top: float = 50) -> None:
        self.name = "parcel_ascent"
        if levtype not in ("ml", "pl"):
            raise ValueError(f"parcel_ascent: levtype must be 'ml' or 'pl', got {levtype!r}")
        if (levtype == "ml") != (model_level_AB is not None):
            raise ValueError("parcel_ascent: levtype='ml' needs model_level_AB, levtype='pl' takes no table")
        if parcel not in native_parcel.PARCELS:
            raise ValueError(f"parcel_ascent: parcel must be one of {', '.join(map(repr, native_parcel.PARCELS))}, got {parcel!r}")
        outputs = {"cape": "cape", "cin": "cin", "plcl": "plcl"} if outputs is None else outputs
        if not isinstance(outputs, dict) or not outputs or not all(isinstance(v, str) for v in outputs.values()):
            raise ValueError(f"parcel_ascent: outputs must be a non-empty dict of output -> param, got {outputs!r}")
        unknown = [name for name in outputs if name not in native_parcel.OUTPUTS]
        if unknown:
            raise ValueError(f"parcel_ascent: unknown outputs {unknown}: the outputs are {', '.join(native_parcel.OUTPUTS)}")
        if not (np.isfinite(float(depth)) and float(depth) >= 0 and np.isfinite(float(top)) and float(top) >= 0):
            raise ValueError(f"parcel_ascent: depth and top must be pressures in hPa, >= 0, got {depth!r} and {top!r}")
        self.outputs = {str(k): v for k, v in outputs.items()}
        self.params = [temperature, specific_humidity]
        if surface_pressure in self.params or temperature == specific_humidity:
            raise ValueError(f"parcel_ascent: temperature, specific_humidity and surface_pressure must be three params, got {self.params + [surface_pressure]}")
        self.levtype, self.parcel, self.surface_pressure = levtype, parcel, surface_pressure
        self.depth_pa, self.top_pa = float(depth) * 100.0, float(top) * 100.0
        if levtype == "ml":
            self._set_table(self.name, model_level_AB)
        say_once(LOG, (type(self), "parity"), PARCEL_PARITY_NOTE)

    def __repr__(self) -> str:
        return f"ParcelAscent(outputs={self.outputs}, levtype={self.levtype!r}, parcel={self.parcel!r})"

    _plan = VerticalIntegral._plan  # the same groups: every param on the same levels, one run of the table, one surface pressure

    def _lift(self, group: dict[str, Any]) -> Any:
        """One stack of the group's fields (one type: float32 only if every field is) — t, then q, then sp — one launch."""
        levels, n = group["levels"], len(group["levels"])
        stack = fields_to_stack([*(f for param in self.params for f in group["by_param"][param]), group["sp"]])
        relayout = stack.layout == native.COLUMNS and PARCEL_COLUMNS_ROUTE[self.levtype] == "fields"
        if relayout:
            stack = stack.to_layout(native.FIELDS)
        rows = lambda first: stack.data[:, first:first + n] if stack.layout == native.COLUMNS else stack.data[first:first + n]  # noqa: E731
        t, q = (Stack(rows(first), stack.n_pts, n, stack.layout) for first in (0, n))
        if self.levtype == "ml":
            A, B = (c[levels[0] - 1:levels[-1] + 1] for c in self._coefficients(stack.device))
            table = dict(A=A, B=B)
        else:
            table = dict(levels_pa=[float(v) * 100.0 for v in levels])
        out = lift_parcels(t, q, stack.level_view(2 * n), parcel=self.parcel, depth_pa=self.depth_pa, top_pa=self.top_pa, outputs=tuple(self.outputs), **table)
        return out.to_layout(native.COLUMNS) if relayout else out

    def forward(self, data: Any) -> FieldList:
        passed, plan = self._plan(list(data))
        result = list(passed)
        for group in plan:
            out = self._lift(group)
            for row, param in enumerate(self.outputs.values()):
                result.append(new_field_from_stack(out, row, template=group["sp"], metadata=dict(param=param, levtype="sfc")))
        return FieldList(result)
