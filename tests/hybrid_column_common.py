"""What the tests of the two kernels on hybrid model-level columns share (``atx_levels_interpolate``, ``atx_geopotential_on_model_levels``):
the storage shapes of the GPU tests and how they are allocated, the bit comparison and the A / B table of the two restatements, and the
FieldList builder of the two host tests.  It shares no code with the package.
"""

from __future__ import annotations

import numpy as np
import pytest

WIDTHS = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
# the 16-byte route; an odd pitch and an unaligned base for the scalar route
COLUMN_STORAGE = ("columns", "columns-pitch+1", "columns-base+1")
# the field-major kernel, tight and with a pitch
FIELD_STORAGE = ("fields", "fields-pitch+3")
CANARY = 7.25


def allocate(rows: int, row_len: int, storage: str, dtype, dev, fill: float):
    """A ``[rows, pitch]`` view on the device, every element ``fill``: "pitch+1" is a pitch that is no multiple of the 16-byte vector,
    "base+1" keeps the aligned pitch and starts one element into a larger allocation.  ``rows`` may be 0."""
    import torch

    per16 = 16 // np.dtype(dtype).itemsize
    pitch = -(-max(row_len, 1) // per16) * per16
    if storage == "columns-pitch+1":
        pitch = pitch + 1
    if storage == "fields":
        pitch = row_len
    if storage == "fields-pitch+3":
        pitch = row_len + 3
    off = 1 if storage == "columns-base+1" else 0
    flat = torch.full((rows * pitch + per16 + off,), fill, dtype=torch.float32 if dtype is np.float32 else torch.float64, device=dev)
    data = flat[off: off + rows * pitch].view(rows, pitch) if rows * pitch else flat[:0].view(rows, pitch)
    if rows * pitch:
        assert (data.data_ptr() % 16 != 0) == (off == 1)
    return data


def bits_type(T):
    return np.uint32 if np.dtype(T).itemsize == 4 else np.uint64


def assert_same_bits(got: np.ndarray, want: np.ndarray, what: str, axes: str) -> None:
    """NaN exactly where the statement has NaN (which NaN is unspecified), the statement's bits everywhere else.  ``axes`` names what an
    index of a failure message counts, "(point, level)" say."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {axes} {np.argwhere(gn != wn)[:5].tolist()}"
    same = (np.ascontiguousarray(got).view(bits_type(got.dtype)) == np.ascontiguousarray(want).view(bits_type(want.dtype))) | wn
    assert same.all(), f"{what}: bits differ at {axes} {np.argwhere(~same)[:5].tolist()}"


def eta_table(n_half: int, of: int | None = None, bend: float = 20000.0) -> tuple[np.ndarray, np.ndarray]:
    """B = eta^2, A = bend eta (1 - eta), eta = k / of for k = 0 .. n_half - 1: the top half level at p = 0 (``of`` defaults to
    n_half - 1: the last half level is the ground, A = 0 and B = 1 there; a larger ``of`` is a table cut off above the ground, with
    A[H - 1] != 0).  With ``bend`` = 150 000 the pressure DECREASES towards the ground wherever sp < 75 000 Pa: columns that are not
    monotone, which the levels statement counts whole."""
    of = n_half - 1 if of is None else of
    eta = np.arange(n_half, dtype=np.float64) / np.float64(of)
    return np.float64(bend) * eta * (np.float64(1.0) - eta), eta * eta


def fields(*specs, date=20260101):
    """(param, levtype, levelist) specs as a FieldList of 6-point fields with a MARS namespace."""
    from anemoi_transform_amd.fields import fieldlist_from_dicts

    lat, lon = np.linspace(50.0, 0.0, 6), np.linspace(0.0, 50.0, 6)
    out = []
    for param, levtype, levelist in specs:
        spec = dict(values=np.full(6, 100000.0 if param in ("sp", "lnsp") else 250.0), latitudes=lat, longitudes=lon, param=param, levtype=levtype,
                    date=date, time=0, step=0)
        if levelist is not None:
            spec["levelist"] = levelist
        out.append(spec)
    return fieldlist_from_dicts(out, mars=True)
