"""HEALPix pixel indices on the device: ``atx_healpix_ang2pix`` (csrc/atx_healpix.hip) through ``healpix.ang2pix`` and the ``add_healpix``
filter, held against the reference's literals (tests/golden/healpix.json) and the numpy restatement (tests/healpix_restatement.py).

Everything of the statement but cos / sin of theta is plain float64 arithmetic with numpy's bits, so for every row the restatement gives
the SET of indices obtained with numpy's ``z`` and ``sth`` each moved by -2 .. +2 ulps (``sincos_moderate`` is held to at most 1 ulp from
glibc; two is twice that).  Where the set has one member the kernel must equal it, elsewhere it must be in the set; at most 1 row in
1000 may have more than one member (0 of 4099 have, for every nside and both orderings, on the committed seed).
"""

from __future__ import annotations

import logging

import numpy as np
import pytest
import torch

import healpix_restatement as R
from anemoi_transform_amd import healpix, native, obs
from anemoi_transform_amd.filters import create_filter_by_name

pytestmark = pytest.mark.gpu

ROWS = R.ROWS  # wave and block edges, a partial last block, more than one block
GOLDEN = R.load_golden()
LAT, LON = np.array(GOLDEN["latitude"]), np.array(GOLDEN["longitude"])
NAME = "healpix_idx_16"
_SETS: dict = {}


def _dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random_sets(nside: int, nest: bool) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(lon, lat, candidates)`` of the largest launch, once per process; a launch of n rows takes the first n."""
    key = (nside, nest)
    if key not in _SETS:
        lon, lat = R.random_rows(max(ROWS))
        sets = R.candidates(nside, lon, lat, nest)
        assert (~(sets == sets[0]).all(axis=0)).sum() <= lon.size // 1000  # the condition; test_healpix_host.py checks it without a GPU
        _SETS[key] = (lon, lat, sets)
    return _SETS[key]


# ---- the reference's literals -----------------------------------------------------------------------------------------------------
def _check_filter_output(out, table, kind):
    assert list(out)[-1] == NAME and list(out)[:-1] == list(table)
    col = out[NAME]
    if kind == "device":
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in out.values()) and col.dtype == torch.int64
        col = col.cpu().numpy()
    else:
        col = np.asarray(col)
        assert col.dtype == np.int64
    assert col.tolist() == GOLDEN["healpix_idx_16"]
    assert NAME not in table and out is not table  # the caller's table is as it was


def test_filter_gives_the_reference_literals_on_a_dataframe():
    pd = pytest.importorskip("pandas")
    df = pd.DataFrame({"latitude": LAT, "longitude": LON})
    before = df.copy()
    out = create_filter_by_name("add_healpix", nside=16)(df)
    assert isinstance(out, pd.DataFrame) and tuple(out.columns) == ("latitude", "longitude", NAME) and out.shape == (9, 3)
    _check_filter_output(out, df, "frame")
    assert df.equals(before) and out[["latitude", "longitude"]].equals(before)
    assert out[NAME].equals(pd.Series(GOLDEN["healpix_idx_16"], name=NAME))  # the reference's own assertion


def test_filter_gives_the_reference_literals_on_a_dict_of_arrays():
    table = {"latitude": LAT.copy(), "value": np.arange(9.0), "longitude": LON.copy()}
    out = create_filter_by_name("add_healpix", nside=16)(table)
    assert isinstance(out, dict) and isinstance(out[NAME], np.ndarray) and out["value"] is table["value"]
    _check_filter_output(out, table, "host")
    assert np.array_equal(table["latitude"], LAT) and np.array_equal(table["longitude"], LON) and list(table) == ["latitude", "value", "longitude"]


def test_filter_keeps_a_table_of_device_tensors_on_the_device():
    table = {"latitude": _dev(LAT), "longitude": _dev(LON), "value": _dev(np.arange(9.0))}
    out = create_filter_by_name("add_healpix", nside=16)(table)
    _check_filter_output(out, table, "device")
    assert out["latitude"] is table["latitude"] and torch.equal(table["latitude"].cpu(), torch.from_numpy(LAT))


def test_healpix_grid_through_the_device_search_gives_the_h16_literals():
    """``obs.nearest_grid_index`` over ``healpix.grid(16)`` is what ``assign_to_grid`` / ``superob`` would do for ``"h16"``: the grid
    names need nothing more than wiring."""
    distance, index = obs.nearest_grid_index(*healpix.grid(16), LAT, LON)
    assert np.asarray(index).tolist() == GOLDEN["grid_index_h16"]
    assert np.allclose(distance, GOLDEN["distance"])


# ---- random rows --------------------------------------------------------------------------------------------------------------------
def _check_against_sets(got: np.ndarray, sets: np.ndarray, what: str) -> None:
    single = (sets == sets[0]).all(axis=0)
    print(f"{what}: {int((~single).sum())} of {got.size} rows have more than one candidate index")
    assert np.array_equal(got[single], sets[len(sets) // 2][single]), what
    assert (sets == got).any(axis=0).all(), what
    assert got.min() >= 0


@pytest.mark.parametrize("n", ROWS)
def test_random_rows_against_the_restatement(n):
    for nest, nsides in ((True, R.NEST_NSIDES), (False, R.RING_NSIDES)):
        for nside in nsides:
            lon, lat, sets = _random_sets(nside, nest)
            got = healpix.ang2pix(nside, _dev(lon[:n]), _dev(lat[:n]), nest=nest)
            assert got.is_cuda and got.dtype == torch.int64 and got.shape == (n,)
            _check_against_sets(got.cpu().numpy(), sets[:, :n], f"n={n} nside={nside} {'nest' if nest else 'ring'}")


def test_special_rows_equal_the_restatement():
    """Branch edges of loc2pix and fmodulo; a row is kept only if its +-2-ulp set has one member."""
    lon, lat = R.special_rows()
    assert R.valid(lon, lat).all()
    for nest, nsides in ((True, R.NEST_NSIDES), (False, R.RING_NSIDES)):
        for nside in nsides:
            sets = R.candidates(nside, lon, lat, nest)
            keep = (sets == sets[0]).all(axis=0)
            what = f"nside={nside} {'nest' if nest else 'ring'}"
            print(f"special rows, {what}: {int(keep.sum())} of {lon.size} kept")
            assert keep.sum() >= 40, what
            got = healpix.ang2pix(nside, lon, lat, nest=nest).cpu().numpy()
            assert np.array_equal(got[keep], R.ang2pix(nside, lon, lat, nest)[keep]), what
            assert (sets == got).any(axis=0).all(), what


# ---- round trip -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nside", [1, 3, 16, 64])
def test_ring_index_of_every_pixel_centre_is_that_pixel(nside):
    lat, lon = healpix.grid(nside)
    n_pix = healpix.npix(nside)
    ring = healpix.ang2pix(nside, lon, lat, nest=False)
    assert torch.equal(ring, torch.arange(n_pix, device=ring.device))
    if nside & (nside - 1) == 0:
        nest = healpix.ang2pix(nside, lon, lat, nest=True)
        assert torch.equal(torch.sort(nest).values, torch.arange(n_pix, device=nest.device))  # a permutation


# ---- rows without a pixel -----------------------------------------------------------------------------------------------------------
def test_rows_without_a_pixel():
    lon, lat = R.random_rows(257)
    lon, lat = lon.copy(), lat.copy()
    bad = [3, 64, 130, 256]
    lat[3], lat[64], lat[130], lon[256] = np.nan, 90.0001, -91.0, np.inf
    with pytest.raises(ValueError, match=r"\b4 of 257 rows"):
        healpix.ang2pix(16, lon, lat)
    with pytest.raises(ValueError, match=r"\b4 of 257 rows"):
        create_filter_by_name("add_healpix", nside=16)({"latitude": lat, "longitude": lon})
    for nest in (True, False):
        out = torch.full((257,), -7, dtype=torch.int64, device="cuda")
        n_bad = torch.full((1,), 99, dtype=torch.int64, device="cuda")  # the call sets it, whatever it held
        native.healpix_ang2pix(_dev(lon), _dev(lat), 16, nest, out, n_bad)
        got = out.cpu().numpy()
        assert int(n_bad.item()) == 4 and (got[bad] == -1).all()
        good = np.setdiff1d(np.arange(257), bad)
        assert np.array_equal(got[good], healpix.ang2pix(16, lon[good], lat[good], nest=nest).cpu().numpy())
        assert np.array_equal(got, np.where(R.valid(lon, lat), got, -1)) and (got[good] >= 0).all()
    lon[256] = -np.inf
    lat[0] = np.inf
    with pytest.raises(ValueError, match=r"\b5 of 257 rows"):
        healpix.ang2pix(16, lon, lat, nest=False)


def test_arguments_are_checked_before_the_launch():
    with pytest.raises(ValueError, match="power of 2"):
        healpix.ang2pix(12, LON, LAT)
    assert healpix.ang2pix(12, LON, LAT, nest=False).shape == (9,)  # RING takes any nside
    with pytest.raises(ValueError, match="nside"):
        healpix.ang2pix(0, LON, LAT)
    with pytest.raises(ValueError, match="differ in length"):
        healpix.ang2pix(16, LON[:5], LAT)
    empty = healpix.ang2pix(16, np.zeros(0), np.zeros(0))
    assert empty.shape == (0,) and empty.dtype == torch.int64


# ---- column kinds ---------------------------------------------------------------------------------------------------------------------
def test_strided_and_float32_columns_equal_their_float64_copies():
    lon, lat = R.random_rows(4099)
    block = _dev(np.stack([lon, lat], axis=1))  # [n, 2]: both columns have stride 2
    assert not block[:, 0].is_contiguous()
    want = healpix.ang2pix(16, _dev(lon), _dev(lat))
    assert torch.equal(healpix.ang2pix(16, block[:, 0], block[:, 1]), want)
    lon32, lat32 = _dev(lon.astype(np.float32)), _dev(lat.astype(np.float32))
    assert torch.equal(healpix.ang2pix(16, lon32, lat32), healpix.ang2pix(16, lon32.double().contiguous(), lat32.double().contiguous()))
    assert torch.equal(healpix.ang2pix(16, lon.astype(np.float32), lat.astype(np.float32)), healpix.ang2pix(16, lon32, lat32))


# ---- the parity note ------------------------------------------------------------------------------------------------------------------
def test_parity_note_is_said_once(caplog):
    from anemoi_transform_amd.core import reset_notes

    reset_notes()
    with caplog.at_level(logging.DEBUG, logger="anemoi_transform_amd"):
        healpix.ang2pix(16, LON, LAT)
        create_filter_by_name("add_healpix", nside=16)({"latitude": LAT, "longitude": LON})
    notes = [r for r in caplog.records if "healpy's ang2pix is restated" in r.getMessage()]
    assert len(notes) >= 2 and notes[0].levelno == logging.WARNING and all(r.levelno == logging.DEBUG for r in notes[1:])
