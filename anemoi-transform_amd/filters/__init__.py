"""The filter plugin registry of the hot path (mirror of R: filters/__init__.py:19-64).

Registered names:
  field filters   regrid, apply_mask_fields, remove_nans_fields, rescale, convert,
                  orog_to_z_fields, z_to_orog_fields, clip_fields, impute_nans_fields,
                  lnsp_to_sp, sp_to_lnsp, glacier_mask, noop,
                  snow_depth_m, snow_cover, cos_sin_from_rad, cos_sin_mean_wave_direction,
                  w_to_wz, wz_to_w, uv_to_ddff, ddff_to_uv, sum, accum_to_interval   (multi-input, filters/multi.py)
                  rodeo_opera_clipping, rodeo_opera_preprocessing, oras6_clipping, land_parameters,
                  r_to_d, d_to_r, q_to_r, r_to_q, q_to_r_height_with_p, r_to_q_height_with_p
                                                             (multi-input, filters/domain.py)
                  rotate_winds, unrotate_winds               (vector frames, filters/winds.py)
                  ml_to_pl                                   (model levels to pressure levels, filters/vertical.py)
  tabular         irregular_to_grid, assign_to_grid, superob (observation tables onto a grid, filters/tabular.py)
                  add_forcings, add_azimuth, add_msg_angles, radiance_to_brightness_temperature, add_healpix,
                  fill_orography, geopotential_to_height_tabular, apply_column_transformations
                                                             (per-row columns, filters/tabular.py)
                  sort_by, drop_duplicates, drop             (row sets on the device / column bookkeeping, filters/tabular.py)
                  mask_tabular, mask_outside_range, mask_infs, mask_dewpoint_temperature, exclude_dates,
                  remove_extreme_values, clip_tabular, impute_nans_tabular, drop_nans_tabular
                                                             (QC: masking, clipping, filling, dropping rows; filters/tabular.py)
                  rename_fields, clear_step, repeat_members, earthkitfieldlambda, empty,
                  icon_refinement_level   (re-labelling / re-listing, filters/metadata.py)
  dispatchers     mask (alias apply_mask), remove_nans (alias drop_nans),
                  geopotential_to_height (alias orog_to_z), height_to_geopotential (alias z_to_orog),
                  clip (alias clipper), impute_nans (alias replace_nans), rename

The dispatchers pick the field or the tabular filter from the configuration keys exactly
as the reference does; given a DataFrame — or a plain mapping of columns — ``mask``,
``clip``, ``impute_nans`` and ``remove_nans`` call ``mask_tabular``, ``clip_tabular``,
``impute_nans_tabular`` and ``drop_nans_tabular``, and ``geopotential_to_height`` calls
``geopotential_to_height_tabular`` with its ``geopotential`` and ``height`` keys
(``height`` defaults to ``"orog"`` there, as in the reference).  A configuration that
belongs to the other half raises the reference's "Ambiguous config" ``ValueError``.
``rename`` alone still raises ``NotImplementedError`` for its tabular half.
Observations enter the field path through ``irregular_to_grid`` (with
``assign_to_grid`` before it): a table goes to the device once and comes out as
one HBM stack of gridded fields.  ``sort_by`` and ``drop_duplicates`` reorder and
thin a table by pandas' order and equality on the device, ``drop`` removes columns,
and the nine QC filters mask, clip, fill and drop rows with one program of compares
and selects per row, so a chain that needs them stays a mapping of device tensors.
``filter_query``, ``mask_values_custom``, ``encode_statids`` and the tabular ``rename``
stay out.
"""

from __future__ import annotations

from collections.abc import Mapping
from typing import Any

from ..core import DispatchingFilter, Filter, filter_registry

# importing the modules registers the field filters
from . import masks as _masks  # noqa: E402
from . import domain as _domain  # noqa: E402
from . import metadata as _metadata  # noqa: E402
from . import multi as _multi  # noqa: E402
from . import pointwise as _pointwise  # noqa: E402
from . import regrid as _regrid  # noqa: E402
from . import tabular as _tabular_filters  # noqa: E402
from . import vertical as _vertical  # noqa: E402
from . import winds as _winds  # noqa: E402
from .masks import MaskVariable, RemoveNaNs as RemoveNaNsFields
from .pointwise import Clipper, ImputeNaNs as ImputeNaNsFields, Orography
from .tabular import ClipTabular, DropNaNsTabular, GeopotentialToHeightTabular, ImputeNaNsTabular, MaskValues


class _TableFallback:
    """A table is a DataFrame or a plain mapping name -> column (filters/tabular.py): the mapping takes the tabular half too."""

    def forward_fallback(self, data: Any) -> Any:
        if isinstance(data, Mapping):
            return self.forward_tabular(data)
        return super().forward_fallback(data)


class Mask(_TableFallback, DispatchingFilter):
    """R: filters/mask.py:19-35."""

    def __init__(self, **config: Any) -> None:
        if "path" in config or "mask_param" in config:
            self.filter = MaskVariable(**config)
        else:
            self.filter = MaskValues(**config)

    def forward_fields(self, data: Any) -> Any:
        return self.filter.forward(data)

    def forward_tabular(self, data: Any) -> Any:
        return self.filter.forward(data)


class RemoveNaNs(_TableFallback, DispatchingFilter):
    """R: filters/remove_nans.py:19-47."""

    def __init__(self, **config: Any) -> None:
        if len(config) == 0:  # valid for both
            self.tabular_filter = DropNaNsTabular()
            self.field_filter = RemoveNaNsFields()
        elif ("columns" in config) or ("column_prefix" in config) or ("how" in config):
            self.tabular_filter = DropNaNsTabular(**config)
            self.field_filter = None
        else:
            self.tabular_filter = None
            self.field_filter = RemoveNaNsFields(**config)

    def forward_fields(self, data: Any) -> Any:
        if self.field_filter is None:
            raise ValueError("Ambigious config for RemoveNaNs filter.")
        return self.field_filter.forward(data)

    def forward_tabular(self, data: Any) -> Any:
        if self.tabular_filter is None:
            raise ValueError("Ambigious config for RemoveNaNs filter.")
        return self.tabular_filter.forward(data)


class GeopotentialToHeight(_TableFallback, DispatchingFilter):
    """R: filters/geopotential_to_height.py:19-47."""

    def __init__(self, **config: Any) -> None:
        config["geopotential"] = config.get("geopotential", "z")
        if ("height" in config) and ("orography" in config):
            raise ValueError("Must specify either 'height' or 'orography' parameter, but not both.")
        if "height" not in config:
            config["height"] = config.pop("orography", "orog")
        self.field_filter = Orography(geopotential=config["geopotential"], orography=config["height"])
        self.tabular_filter = GeopotentialToHeightTabular(geopotential=config["geopotential"], height=config["height"])

    def forward_fields(self, data: Any) -> Any:
        return self.field_filter.forward(data)

    def backward_fields(self, data: Any) -> Any:
        return self.field_filter.backward(data)

    def forward_tabular(self, data: Any) -> Any:
        return self.tabular_filter.forward(data)

    def patch_data_request(self, data_request: dict) -> dict:
        return self.field_filter.patch_data_request(data_request)


class Clip(_TableFallback, DispatchingFilter):
    """R: filters/clip.py:19-35."""

    def __init__(self, **config: Any) -> None:
        if "param" in config and isinstance(config["param"], str):
            self.filter = Clipper(**config)
        else:
            self.filter = ClipTabular(**config)

    def forward_fields(self, data: Any) -> Any:
        return self.filter.forward(data)

    def forward_tabular(self, data: Any) -> Any:
        return self.filter.forward(data)


class ImputeNaNs(_TableFallback, DispatchingFilter):
    """R: filters/impute_nans.py:19-49."""

    def __init__(self, **config: Any) -> None:
        if len(config) == 0:
            self.tabular_filter = ImputeNaNsTabular()  # raises like the reference: required inputs are missing
            self.field_filter = ImputeNaNsFields()
        elif ("columns" in config) or ("column_prefix" in config):
            self.tabular_filter = ImputeNaNsTabular(**config)
            self.field_filter = None
        else:
            self.tabular_filter = None
            self.field_filter = ImputeNaNsFields(**config)

    def forward_fields(self, data: Any) -> Any:
        if self.field_filter is None:
            raise ValueError("Ambiguous config for ImputeNaNs field filter.")
        return self.field_filter.forward(data)

    def forward_tabular(self, data: Any) -> Any:
        if self.tabular_filter is None:
            raise ValueError("Ambiguous config for ImputeNans tabular filter.")
        return self.tabular_filter.forward(data)


filter_registry.register("mask", Mask, aliases=["apply_mask"])
filter_registry.register("remove_nans", RemoveNaNs, aliases=["drop_nans"])
filter_registry.register("geopotential_to_height", GeopotentialToHeight, aliases=["orog_to_z"])
filter_registry.register("height_to_geopotential", GeopotentialToHeight.reversed, aliases=["z_to_orog"])
filter_registry.register("clip", Clip, aliases=["clipper"])
filter_registry.register("impute_nans", ImputeNaNs, aliases=["replace_nans"])


def create_filter_by_name(name: str, *, context: Any = None, **config: Any) -> Filter:
    """R: filters/__init__.py:36-40."""
    filter = filter_registry.create(name, **config)
    filter.context = context
    return filter


def create_filter(context: Any, config: Any) -> Filter:
    """R: filters/__init__.py:43-60 — ``config`` is ``"name"`` or ``{"name": {kwargs}}``."""
    filter = filter_registry.from_config(config)
    filter.context = context
    return filter


__all__ = ["filter_registry", "create_filter", "create_filter_by_name"]
